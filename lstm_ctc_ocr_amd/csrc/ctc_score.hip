// Lexicon scoring under CTC for gfx950: costs[n][k] = -log p(candidate k | logits of sample n) for K candidate strings against ONE set of
// logits [T, N, C], the arg-min per sample and the lexicon's log-normaliser.  The forward half of CTC with the logits shared: the loss kernels
// of ctc.hip take one label per sample (K candidates would mean K copies of the logits) and report an infeasible label as cost 0, which would
// win every arg-min; here an impossible candidate costs +inf.
//
// Three launches, ordered by the stream (no workgroup waits on another); the first and the last are shared with ctc_trie.hip and live in
// ctc_common.h:
//   ctc_score_rows_kernel    lse[t][n] = log sum_c exp(act[t][n][c]) for the rows a sample owns (t < Tn), the row held in registers (16 elements a
//                            thread, as ctc_wide_rows_kernel): one workgroup of 256 / 512 / 1024 threads per row, or, for C <= 1024, one WAVE per
//                            row and four rows per workgroup (no LDS, no barrier).  Rows with t >= Tn are neither read nor written.
//   ctc_score_cands_kernel   one wave per (sample, candidate), four per workgroup.  alpha of the S = 2L+1 slots lives in registers, lane-contiguous
//                            (slot s in lane s / VT, register s % VT); the s-1 / s-2 neighbours are the lane's own registers or come from the lane
//                            below through the DPP wave shift.  No LDS and no barrier.  Per frame a lane gathers act[t][n][label] for its odd slots
//                            and every lane reads the blank's logit and lse[t][n] (one address each); the loads of frame t+1 are issued before the
//                            log-add-exp of frame t.
//   ctc_score_best_kernel    one workgroup per sample: arg-min (lowest index on ties, -1 when no candidate is feasible), its cost, and
//                            log sum_k exp(-cost) (-inf when none is finite).
// Infeasible means +inf, never 0: Tn <= 0, L + repeats > Tn, L outside [0, max_label_len], or a label inside the candidate's length that is
// outside [0, C) or equals the blank.  Such a label is never used as an index, and words beyond a candidate's length are never read.
#include "ctc_common.h"
#include <math.h>

constexpr int SCORE_MAX_LABEL = 255;
constexpr int SCORE_MAX_K = 65536;
constexpr int SCORE_CW = 4;              // candidates (waves) per workgroup of the candidates kernel

// VT = extended-label slots per lane (S = 2L+1 <= 64 * VT for every L <= max_label_len: chosen on the host)
template <int VT>
__global__ __launch_bounds__(64 * SCORE_CW) void ctc_score_cands_kernel(
    const float* __restrict__ act, const float* __restrict__ lse, const int* __restrict__ input_len, const int* __restrict__ cand_labels,
    const int* __restrict__ cand_len, int sample_stride, int T, int N, int C, int K, int Lmax, int blank, float* __restrict__ costs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y, k = blockIdx.x * SCORE_CW + wave;
    if (k >= K) return;                                   // (whole waves; the kernel has no barrier)
    const size_t cand = (size_t)n * sample_stride + k;
    const int L = cand_len[cand];
    const int Tn = min(input_len[n], T);
    float* out = costs + (size_t)n * K + k;
    if (L < 0 || L > Lmax || Tn <= 0) { if (lane == 0) *out = INFINITY; return; }
    const int* labels = cand_labels + cand * Lmax;
    const int S = 2 * L + 1;

    // this lane's slots: the label of an odd slot inside the candidate (words at or beyond L are not read), whether it may take the s-2 step
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
    if (bad || L + rep > Tn) { if (lane == 0) *out = INFINITY; return; }

    const size_t tstride = (size_t)N * C;
    const float* a_n = act + (size_t)n * C;
    const float* lse_n = lse + n;
    // logy of this lane's slots at frame t: gathered logit (odd slots) or the blank's (one address for the wave) minus the row's log-sum-exp
    float g[VT], gb, gl;
#define SCORE_LOAD(t_)                                                                                         \
    do {                                                                                                       \
        const float* row_ = a_n + (size_t)(t_) * tstride;                                                      \
        gb = row_[blank]; gl = lse_n[(size_t)(t_) * N];                                                        \
        _Pragma("unroll") for (int v = 0; v < VT; ++v) {                                                       \
            const bool odd_ = VT > 1 ? (v & 1) : (lane & 1);                                                   \
            g[v] = odd_ ? row_[lab[v]] : 0.f;                                                                  \
        }                                                                                                      \
    } while (0)
#define SCORE_LOGY(dst)                                                                                        \
    _Pragma("unroll") for (int v = 0; v < VT; ++v) {                                                           \
        const bool odd_ = VT > 1 ? (v & 1) : (lane & 1);                                                       \
        dst[v] = in[v] ? (odd_ ? g[v] : gb) - gl : NEG_INF;                                                    \
    }
    float a[VT], ly[VT];
    SCORE_LOAD(0);
    SCORE_LOGY(ly);
#pragma unroll
    for (int v = 0; v < VT; ++v) a[v] = (lane * VT + v < 2) ? ly[v] : NEG_INF;          // (slot 1 of an empty candidate: in[] is false, -inf)
    if (Tn > 1) { SCORE_LOAD(1); SCORE_LOGY(ly); }
    for (int t = 1; t < Tn; ++t) {
        SCORE_LOAD(min(t + 1, Tn - 1));                   // frame t + 1, in flight during the step below
        float p1, p2;
        if constexpr (VT == 1) { p1 = wave_shr1(a[0], NEG_INF); p2 = wave_shr1(p1, NEG_INF); }
        else { p1 = wave_shr1(a[VT - 1], NEG_INF); p2 = wave_shr1(a[VT > 1 ? VT - 2 : 0], NEG_INF); }
        float na[VT];
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const float x1 = v >= 1 ? a[v >= 1 ? v - 1 : 0] : p1;
            const float x2 = v >= 2 ? a[v >= 2 ? v - 2 : 0] : (v == 1 ? p1 : p2);
            na[v] = lse3_flat(a[v], x1, skip[v] ? x2 : NEG_INF) + ly[v];
        }
#pragma unroll
        for (int v = 0; v < VT; ++v) a[v] = na[v];
        SCORE_LOGY(ly);
    }
#undef SCORE_LOAD
#undef SCORE_LOGY
    float e1, e2;
    ctc_last_two<VT>(a, S, e1, e2);
    if (lane == 0) {
        const float m = fmaxf(e1, e2);
        *out = (m == NEG_INF) ? INFINITY : -(m + logf(expf(e1 - m) + expf(e2 - m)));
    }
}

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/ocr_hip.h)
// ------------------------------------------------------------------------------------------
extern "C" int ocr_ctc_score_supported(int alphabet_size, int max_time, int max_label_len, int num_candidates) {
    return alphabet_size >= 1 && alphabet_size <= SCORE_MAX_C && max_time >= 1 && max_label_len >= 0 && max_label_len <= SCORE_MAX_LABEL &&
           num_candidates >= 1 && num_candidates <= SCORE_MAX_K;
}
// the lse[T][N] table
extern "C" int ocr_ctc_score_workspace_size(int alphabet_size, int max_time, int minibatch, size_t* bytes) {
    if (!bytes || minibatch <= 0 || !ocr_ctc_score_supported(alphabet_size, max_time, 0, 1) || (long)minibatch * max_time > 0x7fffffffL)
        return OCR_ERR_INVALID;
    *bytes = ctc_align256((size_t)minibatch * max_time * sizeof(float));
    return OCR_OK;
}
extern "C" int ocr_ctc_score(const float* activations, const int* input_lengths, const int* cand_labels, const int* cand_lengths, int sample_stride,
                             int alphabet_size, int minibatch, int max_time, int num_candidates, int max_label_len, int blank_label, float* costs,
                             int* best, float* best_cost, float* log_norm, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!activations || !input_lengths || !cand_labels || !cand_lengths || !costs || !workspace) return OCR_ERR_INVALID;
    const int outs = (best != nullptr) + (best_cost != nullptr) + (log_norm != nullptr);
    if (outs != 0 && outs != 3) return OCR_ERR_INVALID;
    if (!ocr_ctc_score_supported(alphabet_size, max_time, max_label_len, num_candidates)) return OCR_ERR_INVALID;
    if (blank_label < 0 || blank_label >= alphabet_size || (sample_stride != 0 && sample_stride != num_candidates)) return OCR_ERR_INVALID;
    if (minibatch > 65535) return OCR_ERR_INVALID;        // the candidates launch has the sample in grid.y
    size_t need = 0;
    if (ocr_ctc_score_workspace_size(alphabet_size, max_time, minibatch, &need) != OCR_OK || workspace_bytes < need) return OCR_ERR_INVALID;
    const int C = alphabet_size, N = minibatch, T = max_time, K = num_candidates;
    float* lse = (float*)workspace;

    ctc_score_rows(activations, input_lengths, T, N, C, lse, stream);
    OCR_CHECK_LAUNCH();

    const dim3 grid(ceil_div(K, SCORE_CW), N);
    const int SMAX = smax_for(max_label_len);
#define SCORE_CANDS(V)                                                                                                            \
    ctc_score_cands_kernel<V><<<grid, 64 * SCORE_CW, 0, stream>>>(activations, lse, input_lengths, cand_labels, cand_lengths, sample_stride, T, N, C, K, \
                                                                  max_label_len, blank_label, costs)
    if (SMAX <= 64) SCORE_CANDS(1); else if (SMAX <= 128) SCORE_CANDS(2); else if (SMAX <= 256) SCORE_CANDS(4); else SCORE_CANDS(8);
#undef SCORE_CANDS
    OCR_CHECK_LAUNCH();

    if (outs == 3) {
        ctc_score_best(costs, N, K, best, best_cost, log_norm, stream);
        OCR_CHECK_LAUNCH();
    }
    return OCR_OK;
}

// Shallow fusion after the fact: costs[n][k] -= lm_score[n][k] in place (a candidate's CTC cost minus what a language model or constraint
// adds to its log-probability; an empty slot is +inf - (-inf) = +inf), then best / best_cost / log_norm of the fused costs as ocr_ctc_score
// computes them.  With lm_score all zero the costs keep their bits and the three outputs are ocr_ctc_score's.
__global__ __launch_bounds__(256) void ctc_score_fuse_kernel(float* __restrict__ costs, const float* __restrict__ lm_score, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) costs[i] = costs[i] - lm_score[i];
}
extern "C" int ocr_ctc_score_fuse(float* costs, const float* lm_score, int minibatch, int num_candidates, int* best, float* best_cost,
                                  float* log_norm, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!costs || !lm_score || !best || !best_cost || !log_norm) return OCR_ERR_INVALID;
    if (minibatch < 1 || minibatch > 65535 || num_candidates < 1 || num_candidates > SCORE_MAX_K) return OCR_ERR_INVALID;
    const size_t total = (size_t)minibatch * num_candidates;
    ctc_score_fuse_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(costs, lm_score, total);
    OCR_CHECK_LAUNCH();
    ctc_score_best(costs, minibatch, num_candidates, best, best_cost, log_norm, stream);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
