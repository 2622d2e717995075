// CTC forced alignment for gfx950: the best (Viterbi) alignment of K candidate strings against ONE set of logits [T, N, C].  Per (sample,
// candidate) and character j: start[j] / end[j] = the first and last frame the best path spends on it, score[j] = the sum of
// act[t][n][label_j] - lse[t][n] over those frames, and path_cost = minus the log-probability of the best path.  The max-plus twin of
// ctc_score_cands_kernel (ctc_score.hip) plus back-pointers and a back-trace.  Operands, limits and the meaning of "infeasible" are
// ocr_ctc_score's; an infeasible candidate gets -1 / -1 / -inf in all max_label_len slots and path_cost +inf, a feasible one -1 / -1 / -inf in
// the slots at and beyond its length.
//
// Two launches, ordered by the stream:
//   ctc_score_rows_kernel   (ctc_common.h) lse[t][n] into the head of the workspace, the launch and layout of ocr_ctc_score.
//   ctc_align_kernel        one wave per (sample, candidate), four per workgroup, no workgroup barrier.
//     forward     v of the S = 2L+1 slots in registers, slot s in lane s / VT, register s % VT, neighbours through the DPP wave shift, the loads
//                 of frame t+1 in flight during step t: v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if the skip is allowed) + ly with
//                 ly = act - lse rounded once; no exp, no log, so a host model reproduces every bit.  The step taken (0, 1 or 2: a larger step
//                 replaces a smaller one only when its value is strictly greater) is two bits; a lane packs its VT steps into one 16-bit word
//                 per frame.
//     back-pointer words   With Tn <= 64 they stay in LDS ([frame][lane], 8 KiB a wave).  With Tn > 64 every frame's 64 words go to the
//                 workspace behind the lse table (one coalesced 128-byte store per frame) and come back in blocks of 64 frames, 16 bytes a lane
//                 per load.  Either way the walk reads LDS only.
//     back-trace  per block of 64 frames, last block first: each lane loads ITS column of 16 rows (addresses that do not depend on the path),
//                 then the walk picks the word of lane s / VT with v_readlane and keeps the slot in a scalar register: no step of the serial
//                 walk waits on memory, global or LDS.  Lane i keeps the slot of frame t0 + i; with its neighbours' slots (DPP shifts, the
//                 slots across the block edges carried) it sees whether its frame opens or closes a character's span and writes that frame
//                 number into the wave's start / end table in LDS: every entry has one writer.
//     outputs     lane j, j + 64, ... : character j's span from that table, its score summed over the span's frames in ascending t, the
//                 -1 / -1 / -inf fill beyond the length; lane 0 writes path_cost.  Every output word is written exactly once, by a vector
//                 store; no atomics.
// The path ends in slot S-1 unless v[Tn-1][S-2] is strictly greater.
//
// Beyond the tested shapes: any max_time >= 1 runs (the walk is blockwise, LDS use does not depend on T); what grows is the workspace,
// 128 bytes per (sample, candidate, frame) when max_time > 64 (nothing at or below 64): ocr_ctc_align_workspace_size refuses sizes above
// 2^40 bytes.
#include "ctc_common.h"
#include <math.h>

constexpr int ALIGN_MAX_C = SCORE_MAX_C;
constexpr int ALIGN_MAX_LABEL = 255;
constexpr int ALIGN_MAX_K = 65536;
constexpr int ALIGN_CW = 4;               // candidates (waves) per workgroup
constexpr int ALIGN_BLOCK = 64;           // frames per back-trace block
constexpr int ALIGN_CHUNK = 16;           // rows of a block a lane holds in registers while the walk crosses them

__device__ __forceinline__ int align_shr1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int align_shl1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false); }
// the wave's own LDS traffic: a lane's stores before the other lanes' loads
__device__ __forceinline__ void align_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the fill of the slots j0 <= j < Lmax of one (sample, candidate) by its wave
__device__ __forceinline__ void align_fill(int* start, int* end, float* score, int j0, int Lmax, int lane) {
    for (int j = j0 + lane; j < Lmax; j += 64) { start[j] = -1; end[j] = -1; score[j] = NEG_INF; }
}

template <int VT>
__global__ __launch_bounds__(64 * ALIGN_CW) void ctc_align_kernel(
    const float* __restrict__ act, const float* __restrict__ lse, const int* __restrict__ input_len, const int* __restrict__ cand_labels,
    const int* __restrict__ cand_len, int sample_stride, int T, int N, int C, int K, int Lmax, int blank, uint16_t* __restrict__ bp_all,
    int* __restrict__ start_all, int* __restrict__ end_all, float* __restrict__ score_all, float* __restrict__ cost_all) {
    constexpr int LCAP = 32 * VT;                         // L <= (64 VT - 1) / 2 < 32 VT
    __shared__ __attribute__((aligned(16))) uint16_t s_bp[ALIGN_CW][ALIGN_BLOCK * 64];          // (staged 16 bytes a lane)
    __shared__ int s_span[ALIGN_CW][2][LCAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y, k = blockIdx.x * ALIGN_CW + wave;
    if (k >= K) return;                                   // (whole waves; the kernel has no workgroup barrier)
    const size_t cand = (size_t)n * sample_stride + k, pair = (size_t)n * K + k;
    const int L = cand_len[cand];
    const int Tn = min(input_len[n], T);
    int* o_start = start_all + pair * Lmax;
    int* o_end = end_all + pair * Lmax;
    float* o_score = score_all + pair * Lmax;
    float* o_cost = cost_all + pair;
    if (L < 0 || L > Lmax || Tn <= 0) {
        align_fill(o_start, o_end, o_score, 0, Lmax, lane);
        if (lane == 0) *o_cost = INFINITY;
        return;
    }
    const int* labels = cand_labels + cand * Lmax;
    const int S = 2 * L + 1;

    // this lane's slots, as ctc_score_cands_kernel sets them up
    int lab[VT];
    bool skip[VT], in[VT];
    int bad = 0, rep = 0;
#pragma unroll
    for (int v = 0; v < VT; ++v) {
        const int s = lane * VT + v, j = s >> 1;
        const bool odd = VT > 1 ? (v & 1) : (lane & 1);
        const bool has = odd && j < L;
        const int c = has ? labels[j] : blank;
        const int before = (has && j >= 1) ? labels[j - 1] : -1;
        if (has && ((unsigned)c >= (unsigned)C || c == blank)) bad = 1;
        if (has && j >= 1 && c == before) rep++;
        in[v] = s < S;
        skip[v] = has && j >= 1 && c != before;
        lab[v] = (has && (unsigned)c < (unsigned)C) ? c : blank;          // an out-of-range label is never an index
    }
    bad = __any(bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rep += __shfl_xor(rep, o, 64);
    if (bad || L + rep > Tn) {
        align_fill(o_start, o_end, o_score, 0, Lmax, lane);
        if (lane == 0) *o_cost = INFINITY;
        return;
    }

    const size_t tstride = (size_t)N * C;
    const float* a_n = act + (size_t)n * C;
    const float* lse_n = lse + n;
    const bool in_lds = Tn <= ALIGN_BLOCK;                // the back-pointer words never leave LDS
    uint16_t* bp_w = s_bp[wave];
    uint16_t* bp_g = bp_all + pair * (size_t)T * 64;      // (not touched when in_lds: with max_time <= 64 there is no such region)
    float g[VT], gb, gl;
#define ALIGN_LOAD(t_)                                                                                         \
    do {                                                                                                       \
        const float* row_ = a_n + (size_t)(t_) * tstride;                                                      \
        gb = row_[blank]; gl = lse_n[(size_t)(t_) * N];                                                        \
        _Pragma("unroll") for (int v = 0; v < VT; ++v) {                                                       \
            const bool odd_ = VT > 1 ? (v & 1) : (lane & 1);                                                   \
            g[v] = odd_ ? row_[lab[v]] : 0.f;                                                                  \
        }                                                                                                      \
    } while (0)
#define ALIGN_LOGY(dst)                                                                                        \
    _Pragma("unroll") for (int v = 0; v < VT; ++v) {                                                           \
        const bool odd_ = VT > 1 ? (v & 1) : (lane & 1);                                                       \
        dst[v] = in[v] ? (odd_ ? g[v] : gb) - gl : NEG_INF;                                                    \
    }
    float a[VT], ly[VT];
    ALIGN_LOAD(0);
    ALIGN_LOGY(ly);
#pragma unroll
    for (int v = 0; v < VT; ++v) a[v] = (lane * VT + v < 2) ? ly[v] : NEG_INF;
    if (Tn > 1) { ALIGN_LOAD(1); ALIGN_LOGY(ly); }
    for (int t = 1; t < Tn; ++t) {
        ALIGN_LOAD(min(t + 1, Tn - 1));                   // frame t + 1, in flight during the step below
        float p1, p2;
        if constexpr (VT == 1) { p1 = wave_shr1(a[0], NEG_INF); p2 = wave_shr1(p1, NEG_INF); }
        else { p1 = wave_shr1(a[VT - 1], NEG_INF); p2 = wave_shr1(a[VT > 1 ? VT - 2 : 0], NEG_INF); }
        float na[VT];
        unsigned word = 0;
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const float x1 = v >= 1 ? a[v >= 1 ? v - 1 : 0] : p1;
            const float x2 = skip[v] ? (v >= 2 ? a[v >= 2 ? v - 2 : 0] : (v == 1 ? p1 : p2)) : NEG_INF;
            float best = a[v];
            unsigned step = 0;
            if (x1 > best) { best = x1; step = 1; }       // strictly greater: ties prefer staying, then one slot, then two
            if (x2 > best) { best = x2; step = 2; }
            na[v] = best + ly[v];
            word |= step << (2 * v);
        }
        if (in_lds) bp_w[t * 64 + lane] = (uint16_t)word;
        else bp_g[(size_t)t * 64 + lane] = (uint16_t)word;
#pragma unroll
        for (int v = 0; v < VT; ++v) a[v] = na[v];
        ALIGN_LOGY(ly);
    }
#undef ALIGN_LOAD
#undef ALIGN_LOGY
    float e1, e2;
    ctc_last_two<VT>(a, S, e1, e2);
    const bool second = S >= 2 && e2 > e1;                // the path ends in slot S - 1 unless slot S - 2 is strictly better
    if (lane == 0) *o_cost = -(second ? e2 : e1);
    if (L == 0) {                                         // the all-blank path: no spans
        align_fill(o_start, o_end, o_score, 0, Lmax, lane);
        return;
    }

    // ---- back-trace
    int* sp_start = s_span[wave][0];
    int* sp_end = s_span[wave][1];
    for (int j = lane; j < LCAP; j += 64) { sp_start[j] = -1; sp_end[j] = -1; }
    if (!in_lds) __threadfence();                         // the words this wave stored, before any of its lanes loads another lane's
    align_wave_sync();
    int s = __builtin_amdgcn_readfirstlane(second ? S - 2 : S - 1);          // the slot of the frame the walk stands on (wave-uniform)
    int later = -1;                                       // the slot of the first frame of the block after this one
    for (int t0 = (Tn - 1) / ALIGN_BLOCK * ALIGN_BLOCK; t0 >= 0; t0 -= ALIGN_BLOCK) {
        const int cnt = min(ALIGN_BLOCK, Tn - t0);
        if (!in_lds) {
            align_wave_sync();                            // (the block before: every lane has its rows in registers)
            const uint4* src = (const uint4*)(bp_g + (size_t)t0 * 64);
            uint4* dst = (uint4*)bp_w;
#pragma unroll
            for (int q = 0; q < ALIGN_BLOCK * 64 * 2 / 16 / 64; ++q) {
                const int i = q * 64 + lane;
                if (i < cnt * 8) dst[i] = src[i];         // (8 uint4 per frame: nothing beyond the frames of this sample is read)
            }
            align_wave_sync();
        }
        int mine = -1;                                    // the slot of frame t0 + lane
#pragma unroll 1
        for (int c0 = (cnt - 1) / ALIGN_CHUNK * ALIGN_CHUNK; c0 >= 0; c0 -= ALIGN_CHUNK) {
            int row[ALIGN_CHUNK];
#pragma unroll
            for (int r = 0; r < ALIGN_CHUNK; ++r) row[r] = bp_w[(c0 + r) * 64 + lane];
#pragma unroll
            for (int r = ALIGN_CHUNK - 1; r >= 0; --r) {
                const int i = c0 + r;
                if (i < cnt) {
                    if (lane == i) mine = s;
                    if (t0 + i > 0) {                     // (frame 0 has no step and no word)
                        const int w = __builtin_amdgcn_readlane(row[r], s / VT);
                        s -= (w >> (2 * (s & (VT - 1)))) & 3;
                        s = max(s, 0);                    // (a slot never leaves [0, S) on finite logits; nor does it on any others)
                    }
                }
            }
        }
        // s is now the slot of frame t0 - 1
        const int before = align_shr1(mine, t0 > 0 ? s : -1);
        const int after = align_shl1(mine, later);
        if (lane < cnt && (mine & 1)) {                   // (mine >= 0 here)
            const int j = mine >> 1;
            if (before != mine) sp_start[j] = t0 + lane;
            if (after != mine) sp_end[j] = t0 + lane;
        }
        later = __builtin_amdgcn_readfirstlane(mine);
    }
    align_wave_sync();

    // ---- outputs: a lane per character
    for (int j = lane; j < L; j += 64) {
        const int st = sp_start[j], en = sp_end[j];
        const int c = labels[j];                          // (checked above: inside [0, C), not the blank)
        float sc = 0.f;
        const bool whole = st >= 0 && en >= st && en < Tn;          // (always, on finite logits)
        if (whole)
            for (int t = st; t <= en; ++t) sc += a_n[(size_t)t * tstride + c] - lse_n[(size_t)t * N];
        o_start[j] = whole ? st : -1;
        o_end[j] = whole ? en : -1;
        o_score[j] = whole ? sc : NEG_INF;
    }
    align_fill(o_start, o_end, o_score, L, Lmax, lane);
}

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/ocr_hip.h)
// ------------------------------------------------------------------------------------------
extern "C" int ocr_ctc_align_supported(int alphabet_size, int max_time, int max_label_len, int num_candidates) {
    return alphabet_size >= 1 && alphabet_size <= ALIGN_MAX_C && max_time >= 1 && max_label_len >= 0 && max_label_len <= ALIGN_MAX_LABEL &&
           num_candidates >= 1 && num_candidates <= ALIGN_MAX_K;
}
// the lse[T][N] table, then (max_time > 64 only) 64 back-pointer words of 16 bits per (sample, candidate, frame)
extern "C" int ocr_ctc_align_workspace_size(int alphabet_size, int max_time, int minibatch, int num_candidates, int max_label_len, size_t* bytes) {
    if (!bytes || minibatch <= 0 || minibatch > 65535 || !ocr_ctc_align_supported(alphabet_size, max_time, max_label_len, num_candidates) ||
        (long)minibatch * max_time > 0x7fffffffL)
        return OCR_ERR_INVALID;
    const size_t lse_bytes = ctc_align256((size_t)minibatch * max_time * sizeof(float));
    unsigned __int128 bp = 0;
    if (max_time > ALIGN_BLOCK) bp = (unsigned __int128)minibatch * num_candidates * max_time * (64 * sizeof(uint16_t));
    if (bp > ((unsigned __int128)1 << 40)) return OCR_ERR_INVALID;
    *bytes = lse_bytes + ctc_align256((size_t)bp);
    return OCR_OK;
}
extern "C" int ocr_ctc_align(const float* activations, const int* input_lengths, const int* cand_labels, const int* cand_lengths, int sample_stride,
                             int alphabet_size, int minibatch, int max_time, int num_candidates, int max_label_len, int blank_label,
                             int* start, int* end, float* score, float* path_cost, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!activations || !input_lengths || !cand_labels || !cand_lengths || !start || !end || !score || !path_cost || !workspace) return OCR_ERR_INVALID;
    if (!ocr_ctc_align_supported(alphabet_size, max_time, max_label_len, num_candidates)) return OCR_ERR_INVALID;
    if (blank_label < 0 || blank_label >= alphabet_size || (sample_stride != 0 && sample_stride != num_candidates)) return OCR_ERR_INVALID;
    size_t need = 0;
    if (ocr_ctc_align_workspace_size(alphabet_size, max_time, minibatch, num_candidates, max_label_len, &need) != OCR_OK || workspace_bytes < need)
        return OCR_ERR_INVALID;                           // (minibatch > 65535 too: the launch has the sample in grid.y)
    const int C = alphabet_size, N = minibatch, T = max_time, K = num_candidates;
    float* lse = (float*)workspace;
    uint16_t* bp = (uint16_t*)((char*)workspace + ctc_align256((size_t)N * T * sizeof(float)));

    ctc_score_rows(activations, input_lengths, T, N, C, lse, stream);
    OCR_CHECK_LAUNCH();

    const dim3 grid(ceil_div(K, ALIGN_CW), N);
    const int SMAX = smax_for(max_label_len);
#define ALIGN_CANDS(V)                                                                                                              \
    ctc_align_kernel<V><<<grid, 64 * ALIGN_CW, 0, stream>>>(activations, lse, input_lengths, cand_labels, cand_lengths, sample_stride, T, N, C, K, \
                                                            max_label_len, blank_label, bp, start, end, score, path_cost)
    if (SMAX <= 64) ALIGN_CANDS(1); else if (SMAX <= 128) ALIGN_CANDS(2); else if (SMAX <= 256) ALIGN_CANDS(4); else ALIGN_CANDS(8);
#undef ALIGN_CANDS
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
