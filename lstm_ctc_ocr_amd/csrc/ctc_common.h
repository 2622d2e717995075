// What the CTC sources (ctc.hip, ctc_long.hip, ctc_score.hip, ctc_trie.hip) share: the log-add-exp forms, a sample's set-up, the frame-parallel pieces of the
// loss kernels (row log-sum-exp, zero-fill, posterior accumulation, gradient-row store), the row-in-registers loader of the chip-wide rows
// kernels, and the host-side sizes more than one file needs.
#pragma once
#include "common.h"

// (NEG_INF and the DPP wave shifts wave_shr1 / wave_shl1 are in common.h)
__device__ __forceinline__ float lse2(float a, float b) {
    float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + logf(expf(a - m) + expf(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    float m = fmaxf(fmaxf(a, b), c);
    if (m == NEG_INF) return NEG_INF;
    return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// hardware exp2 / log2 forms (v_exp_f32, v_log_f32: ~1e-6 relative) for the T-sequential recursions of the fast kernel,
// where the libm expf / logf sequences (about 40 instructions each, three per step) ARE the critical path
__device__ __forceinline__ float lse2_fast(float a, float b) {
    float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m));
}
__device__ __forceinline__ float lse3_fast(float a, float b, float c) {
    float m = fmaxf(fmaxf(a, b), c);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

// log(e^a + e^b + e^c) as straight-line code on the bare v_exp_f32 / v_log_f32: with every input -inf the maximum is replaced by 0, the
// sum is 0 and v_log_f32 returns -inf, so no branch guards the (-inf) - (-inf) case and the VT updates of a step interleave; the sum
// of a finite case lies in [1, 3], so the denormal scaling of __logf is not needed either
__device__ __forceinline__ float lse3_flat(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    const float m0 = (m == NEG_INF) ? 0.f : m;
    constexpr float LOG2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;
    const float sum = __builtin_amdgcn_exp2f((a - m0) * LOG2E) + __builtin_amdgcn_exp2f((b - m0) * LOG2E) + __builtin_amdgcn_exp2f((c - m0) * LOG2E);
    return m0 + __builtin_amdgcn_logf(sum) * LN2;
}

// e1, e2 = alpha of the last two slots S - 1 and S - 2 (-inf when S = 1), in every lane of a wave that keeps slot s in lane s / VT, register s % VT
template <int VT>
__device__ __forceinline__ void ctc_last_two(const float (&a)[VT], int S, float& e1, float& e2) {
    float x1 = NEG_INF, x2 = NEG_INF;
#pragma unroll
    for (int v = 0; v < VT; ++v) {
        if (v == ((S - 1) & (VT - 1))) x1 = a[v];
        if (S >= 2 && v == ((S - 2) & (VT - 1))) x2 = a[v];
    }
    e1 = __shfl(x1, (S - 1) / VT, 64);
    e2 = (S >= 2) ? __shfl(x2, (S - 2) / VT, 64) : NEG_INF;
}

// log sum_k exp(row[k]) of one logit row by one wave, its lanes striding the class axis (libm expf / logf: this value is in every cost)
__device__ __forceinline__ float ctc_row_lse(const float* __restrict__ row, int C, int lane) {
    float m = NEG_INF;
    for (int k = lane; k < C; k += 64) m = fmaxf(m, row[k]);
    m = wave_max(m);
    float sum = 0.f;
    for (int k = lane; k < C; k += 64) sum += expf(row[k] - m);
    sum = wave_sum(sum);
    return m + logf(sum);
}

// A sample's set-up by its whole workgroup of nt threads: the label offset (exclusive prefix sum of the label lengths, so no scan launch and
// no offsets array), lab[0 .. cap) = the extended label l' = [b, l1, b, ..., lL, b] with the blank beyond S = 2L+1, and the repeat count.
// -> feasible.  A label longer than the capacity has no table: treated like an infeasible sample.  cnt = two shared ints; ends with a
// __syncthreads().
__device__ __forceinline__ bool ctc_sample_setup(const int* __restrict__ flat_labels, const int* __restrict__ label_len, int n, int L, int Tn, int cap,
                                                 int blank, int* lab, int* cnt, int nt) {
    const int tid = threadIdx.x, S = 2 * L + 1;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    int part = 0;
    for (int i = tid; i < n; i += nt) part += label_len[i];
    if (part) atomicAdd(&cnt[0], part);
    __syncthreads();
    const int* labels = flat_labels + cnt[0];
    const bool fits = L >= 0 && S <= cap;
    int rep = 0;
    for (int s = tid; s < cap; s += nt) {
        const bool in = fits && s < S;
        lab[s] = (in && (s & 1)) ? labels[s >> 1] : blank;
        if (in && (s & 1) && s >= 3 && labels[s >> 1] == labels[(s >> 1) - 1]) rep++;
    }
    if (rep) atomicAdd(&cnt[1], rep);
    __syncthreads();
    return fits && Tn > 0 && L + cnt[1] <= Tn;
}

// zero gradient for the frames t0 <= t < T of a sample (those it does not own; everything when it is infeasible), wave w of nw taking
// frames t0 + w, t0 + w + nw, ...
__device__ __forceinline__ void ctc_zero_frames(float* g_n, bf16_t* gb_n, int t0, int T, int C, size_t tstride, int lane, int w, int nw) {
    for (int t = t0 + w; t < T; t += nw)
        for (int k = lane; k < C; k += 64) {
            if (g_n) g_n[t * tstride + k] = 0.f;
            if (gb_n) gb_n[(size_t)t * C + k] = 0;
        }
}

// posterior of (t, s), <= 1, added to its class's accumulator (LDS float atomic); al, be, ly = alpha, beta, log y of the slot
__device__ __forceinline__ void ctc_posterior_add(float* slot, float al, float be, float ly, float logp) {
    if (al != NEG_INF && be != NEG_INF) atomicAdd(slot, expf(al + be - ly - logp));
}

// gradient element (t, k) of a sample: into its f32 [T][N][C] gradient g_n and / or, times scale, into its bf16 [N][T][C] gradient gb_n (the
// layout / dtype the backward GEMMs read)
__device__ __forceinline__ void ctc_grad_store(float v, float* g_n, bf16_t* gb_n, int t, int k, size_t tstride, int C, float scale) {
    if (g_n) g_n[t * tstride + k] = v;
    if (gb_n) gb_n[(size_t)t * C + k] = f2bf(v * scale);
}
// frame t's gradient row by one wave: softmax (exp(row - lse_t)) minus the per-class posterior sums in wacc
__device__ __forceinline__ void ctc_grad_row(const float* __restrict__ row, float lse_t, const float* wacc, float* g_n, bf16_t* gb_n, int t, size_t tstride,
                                             int C, int lane, float scale) {
    for (int k = lane; k < C; k += 64) ctc_grad_store(expf(row[k] - lse_t) - wacc[k], g_n, gb_n, t, k, tstride, C, scale);
}

// Row in registers (ctc_wide_rows_kernel, ctc_score_rows_kernel): TPR threads hold one row, thread rt of them PER elements as PER / VEC chunks of
// VEC consecutive ones; 8 (two 16-byte loads) and 4 need C % VEC == 0 and a 16-byte aligned tensor, 1 takes any C.  -inf past C and when !live.
template <int TPR, int VEC, int PER>
__device__ __forceinline__ void ctc_load_row(const float* __restrict__ row, int C, int rt, bool live, float (&v)[PER]) {
#pragma unroll
    for (int i = 0; i < PER / VEC; ++i) {
        const int k = (i * TPR + rt) * VEC;
        const bool in = live && k < C;                // (k < C covers k + VEC <= C: C is a multiple of VEC)
        if constexpr (VEC == 1) v[i] = in ? row[k] : NEG_INF;
        else {
#pragma unroll
            for (int q = 0; q < VEC / 4; ++q) {
                const f32x4 x = in ? *(const f32x4*)(row + k + 4 * q) : (f32x4){NEG_INF, NEG_INF, NEG_INF, NEG_INF};
                v[i * VEC + 4 * q] = x.x; v[i * VEC + 4 * q + 1] = x.y; v[i * VEC + 4 * q + 2] = x.z; v[i * VEC + 4 * q + 3] = x.w;
            }
        }
    }
}
// maximum of such a row over its NW waves: per thread, per wave, then through s_max[NW] and one barrier; a row of one wave touches no LDS
template <int NW, int PER>
__device__ __forceinline__ float ctc_row_max(const float (&v)[PER], float* s_max, int lane, int wave) {
    float m = v[0];
#pragma unroll
    for (int j = 1; j < PER; ++j) m = fmaxf(m, v[j]);
    m = wave_max(m);
    if constexpr (NW > 1) {
        if (lane == 0) s_max[wave] = m;
        __syncthreads();
        m = s_max[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, s_max[w]);
    }
    return m;
}
// and the sum of the threads' partial sums, in wave order
template <int NW>
__device__ __forceinline__ float ctc_row_sum(float sum, float* s_sum, int lane, int wave) {
    sum = wave_sum(sum);
    if constexpr (NW > 1) {
        if (lane == 0) s_sum[wave] = sum;
        __syncthreads();
        sum = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += s_sum[w];
    }
    return sum;
}

// ---- host side
constexpr int CTC_NW = 16;        // waves per sample: the frame-parallel phases (log-sum-exp rows, gradient rows) are latency chains per
                                  // row (cross-lane reductions, LDS atomics): 16 waves x 4 rows instead of 4 x 16 rows
static inline int smax_for(int max_label_len) { return 2 * max_label_len + 1; }
static inline size_t ctc_align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// the operands and ranges every loss entry point refuses alike; each adds its own conditions
static inline bool ctc_loss_args_ok(const float* activations, const int* flat_labels, const int* label_lengths, const int* input_lengths,
                                    const float* costs, int alphabet_size, int minibatch, int max_time, int max_label_len, int blank_label) {
    return activations && flat_labels && label_lengths && input_lengths && costs && alphabet_size > 0 && minibatch > 0 && max_time > 0 &&
           max_label_len >= 0 && blank_label >= 0 && blank_label < alphabet_size;
}

// ---- what the lexicon scorers (ctc_score.hip per candidate, ctc_trie.hip per prefix-tree node) share: the lse[t][n] rows launch and the
// arg-min / log-normaliser launch.  Kernels and launchers are templates (the launchers' parameter has no other use) so that only the sources
// that launch them instantiate them: the other CTC objects stay what they were.
constexpr int SCORE_MAX_C = 16384;
constexpr int SCORE_PER = 16;            // row elements a thread of the rows kernel keeps
constexpr int SCORE_WAVE_ROW_C = 64 * SCORE_PER;      // up to here a row fits one wave

// TPR threads hold one row: TPR == NT (one row per workgroup, two barriers) or TPR == 64 (one row per wave, NT / 64 rows per workgroup).
// The row is loaded and reduced by ctc_common.h's row-in-registers helpers.
template <int NT, int TPR, int VEC>
__global__ __launch_bounds__(NT) void ctc_score_rows_kernel(const float* __restrict__ act, const int* __restrict__ input_len, int T, int N, int C,
                                                            float* __restrict__ lse_out) {
    constexpr int RPB = NT / TPR, NW = TPR / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long r = (long)blockIdx.x * RPB + (RPB > 1 ? wave : 0);
    const int rt = RPB > 1 ? lane : tid;                  // thread within the row
    if (r >= (long)T * N) return;                         // (per wave when RPB > 1, per workgroup otherwise: no barrier is skipped by a part)
    const int t = (int)(r / N), n = (int)(r - (long)t * N);
    if (t >= min(input_len[n], T)) return;                // not a frame of this sample: neither read nor written
    const float* row = act + (size_t)r * C;

    float v[SCORE_PER];
    ctc_load_row<TPR, VEC>(row, C, rt, true, v);
    __shared__ float s_max[NW > 1 ? NW : 1], s_sum[NW > 1 ? NW : 1];          // (untouched by the one-wave-per-row form: no LDS, no barrier)
    const float m = ctc_row_max<NW>(v, s_max, lane, wave);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < SCORE_PER; ++j) sum += __expf(v[j] - m);          // (elements past C: exp(-inf) = 0)
    sum = ctc_row_sum<NW>(sum, s_sum, lane, wave);
    if (rt == 0) lse_out[r] = m + logf(sum);
}

template <int NT, int TPR, int VEC>
static void ctc_score_rows_launch(const float* act, const int* il, int T, int N, int C, float* lse, hipStream_t stream) {
    const long rows = (long)T * N;
    ctc_score_rows_kernel<NT, TPR, VEC><<<ceil_div(rows, NT / TPR), NT, 0, stream>>>(act, il, T, N, C, lse);
}
// the rows launch of the lexicon scorers: a wave per row while a wave's registers hold it (no barrier, four rows per workgroup); else the
// smallest workgroup that holds the row.  The caller checks the launch.
template <int INSTANCE = 0>
static inline void ctc_score_rows(const float* activations, const int* input_lengths, int T, int N, int C, float* lse, hipStream_t stream) {
    const bool al16 = ((uintptr_t)activations & 15) == 0;
    const int VEC = (al16 && C % 8 == 0) ? 8 : (al16 && C % 4 == 0) ? 4 : 1;
#define SCORE_ROWS(NT, TPR)                                                                       \
    do {                                                                                          \
        if (VEC == 8) ctc_score_rows_launch<NT, TPR, 8>(activations, input_lengths, T, N, C, lse, stream);       \
        else if (VEC == 4) ctc_score_rows_launch<NT, TPR, 4>(activations, input_lengths, T, N, C, lse, stream);  \
        else ctc_score_rows_launch<NT, TPR, 1>(activations, input_lengths, T, N, C, lse, stream);                \
    } while (0)
    if (C <= SCORE_WAVE_ROW_C) SCORE_ROWS(256, 64);
    else if (C <= 256 * SCORE_PER) SCORE_ROWS(256, 256);
    else if (C <= 512 * SCORE_PER) SCORE_ROWS(512, 512);
    else SCORE_ROWS(1024, 1024);
#undef SCORE_ROWS
}

constexpr int SCORE_BEST_NT = 256;
template <int INSTANCE = 0>
__global__ __launch_bounds__(SCORE_BEST_NT) void ctc_score_best_kernel(const float* __restrict__ costs, int K, int* __restrict__ best,
                                                                       float* __restrict__ best_cost, float* __restrict__ log_norm) {
    constexpr int NW = SCORE_BEST_NT / 64;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* c_n = costs + (size_t)n * K;
    __shared__ float s_c[NW], s_sum[NW];
    __shared__ int s_i[NW];
    float bc = INFINITY;
    int bi = 0x7fffffff;
    for (int k = tid; k < K; k += SCORE_BEST_NT) {
        const float c = c_n[k];
        if (c < bc) { bc = c; bi = k; }                   // (ascending k per thread: strict < keeps the lowest index)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float oc = __shfl_xor(bc, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    if (lane == 0) { s_c[wave] = bc; s_i[wave] = bi; }
    __syncthreads();
    bc = s_c[0]; bi = s_i[0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
        if (s_c[w] < bc || (s_c[w] == bc && s_i[w] < bi)) { bc = s_c[w]; bi = s_i[w]; }
    const bool any = bc < INFINITY;
    float sum = 0.f;
    if (any)
        for (int k = tid; k < K; k += SCORE_BEST_NT) sum += expf(bc - c_n[k]);          // (+inf cost: exp(-inf) = 0)
    sum = wave_sum(sum);
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        sum = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += s_sum[w];
        best[n] = any ? bi : -1;
        best_cost[n] = bc;
        log_norm[n] = any ? logf(sum) - bc : NEG_INF;
    }
}

template <int INSTANCE = 0>
static inline void ctc_score_best(const float* costs, int N, int K, int* best, float* best_cost, float* log_norm, hipStream_t stream) {
    ctc_score_best_kernel<INSTANCE><<<N, SCORE_BEST_NT, 0, stream>>>(costs, K, best, best_cost, log_norm);
}
