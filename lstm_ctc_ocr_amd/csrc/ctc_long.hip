// CTC loss + gradient for long labels (up to 255 characters) and for wide alphabets (up to 16384 classes) on gfx950: the forms beyond the reach
// of ctc.hip's fast kernel (S = 2L+1 <= 64).  Semantics as in ctc.hip's header; the pieces shared with the kernels there are in ctc_common.h.
#include "ctc_common.h"
#include <math.h>

// ------------------------------------------------------------------------------------------------------------------
// Long labels (1 <= L <= 255, S = 2L+1 <= 511): the fast kernel's four phases with VT = 2, 4 or 8 extended-label slots per lane.
//   phases 1, 2, 4  all 16 waves, frame-parallel, as in ctc_fast_kernel
//   phase 3         wave 0 runs alpha while wave 1 runs beta.  Lane l owns the VT consecutive slots s = l * VT + v and keeps them in
//                   registers; a step is VT independent lse3_flat updates, and only the two values that cross a lane boundary move
//                   (two whole-wave DPP shifts).  No barrier and no LDS exchange on the chain; the next step's logy values are loaded
//                   one step ahead, and alpha / beta are only ever stored by these waves.
// Tables logy / alpha / beta are [T][SP], SP = 64 * VT, element (t, s) at t * SP + (s % VT) * 64 + s / VT: what a lane owns is SP / 64
// words 64 apart, so every table access of the recursions and of phase 4 is one conflict-free LDS read or one coalesced 256-B line.
// Slots s >= S hold logy = -inf, which keeps their alpha / beta at -inf without a test on the chain.
// Placement (ctc_long_placement): the three tables live in LDS when they fit beside lse[T], the per-wave class accumulators and the
// extended labels (TLDS); otherwise in the caller's workspace, 3 * T * SP floats per sample.  The workspace is written and read by ONE
// workgroup, ordered by the __syncthreads() between the phases: its pointer is deliberately neither __restrict__ nor const.
// ------------------------------------------------------------------------------------------------------------------

// Phase 3 of the long-label forms (ctc_long_kernel, ctc_wide_samples_kernel) on a filled logy table: wave 0 runs alpha and leaves log p(l|x) in *s_logp
// and the cost in *cost, wave 1 runs beta when a gradient is wanted; the other waves pass through.  The caller's __syncthreads() follows.
template <int VT>
__device__ __forceinline__ void ctc_long_recursions(int lane, int wave, int S, int Tn, int blank, bool want_grad, const int* lab, const float* logy,
                                                    float* alpha, float* beta, float* s_logp, float* cost) {
    constexpr int SP = 64 * VT;
    if (wave == 0) {
        bool skip[VT];
        float a[VT], ly[VT];
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const int s = lane * VT + v;
            skip[v] = s < S && s >= 2 && lab[s] != blank && lab[s] != lab[s - 2];
            a[v] = (s < 2) ? logy[v * 64 + lane] : NEG_INF;
            if (want_grad) alpha[v * 64 + lane] = a[v];
            ly[v] = logy[(size_t)min(1, Tn - 1) * SP + v * 64 + lane];
        }
        for (int t = 1; t < Tn; ++t) {
            float lyn[VT];
            const float* nrow = logy + (size_t)min(t + 1, Tn - 1) * SP + lane;
#pragma unroll
            for (int v = 0; v < VT; ++v) lyn[v] = nrow[v * 64];
            const float p1 = wave_shr1(a[VT - 1], NEG_INF), p2 = wave_shr1(a[VT - 2], NEG_INF);
            float na[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const float x1 = v >= 1 ? a[v >= 1 ? v - 1 : 0] : p1;
                const float x2 = v >= 2 ? a[v >= 2 ? v - 2 : 0] : (v == 1 ? p1 : p2);
                na[v] = lse3_flat(a[v], x1, skip[v] ? x2 : NEG_INF) + ly[v];
            }
            float* arow = alpha + (size_t)t * SP + lane;
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                a[v] = na[v]; ly[v] = lyn[v];
                if (want_grad) arow[v * 64] = a[v];
            }
        }
        float e1, e2;
        ctc_last_two<VT>(a, S, e1, e2);
        if (lane == 0) { const float logp = lse2(e1, e2); *s_logp = logp; *cost = -logp; }
    } else if (wave == 1 && want_grad) {
        bool skip[VT];
        float b[VT], ly[VT];
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const int s = lane * VT + v;
            skip[v] = (s + 2 < S) && lab[s + 2] != blank && lab[s + 2] != lab[s];
            b[v] = (s >= S - 2) ? logy[(size_t)(Tn - 1) * SP + v * 64 + lane] : NEG_INF;    // -inf for s >= S
            beta[(size_t)(Tn - 1) * SP + v * 64 + lane] = b[v];
            ly[v] = logy[(size_t)max(Tn - 2, 0) * SP + v * 64 + lane];
        }
        for (int t = Tn - 2; t >= 0; --t) {
            float lyn[VT];
            const float* nrow = logy + (size_t)max(t - 1, 0) * SP + lane;
#pragma unroll
            for (int v = 0; v < VT; ++v) lyn[v] = nrow[v * 64];
            const float q1 = wave_shl1(b[0], NEG_INF), q2 = wave_shl1(b[1], NEG_INF);
            float nb[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                const float x1 = v + 1 < VT ? b[v + 1 < VT ? v + 1 : 0] : q1;
                const float x2 = v + 2 < VT ? b[v + 2 < VT ? v + 2 : 0] : (v + 2 == VT ? q1 : q2);
                nb[v] = lse3_flat(b[v], x1, skip[v] ? x2 : NEG_INF) + ly[v];
            }
            float* brow = beta + (size_t)t * SP + lane;
#pragma unroll
            for (int v = 0; v < VT; ++v) {
                b[v] = nb[v]; ly[v] = lyn[v];
                brow[v * 64] = b[v];
            }
        }
    }
}

template <int VT, bool TLDS>
__global__ __launch_bounds__(64 * CTC_NW) void ctc_long_kernel(
    const float* __restrict__ act, float* __restrict__ grad, const int* __restrict__ flat_labels,
    const int* __restrict__ label_len, const int* __restrict__ input_len, int T, int N, int C, int blank,
    float* __restrict__ costs, bf16_t* __restrict__ grad_ntc, float scale, float* ws) {
    constexpr int SP = 64 * VT;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    float* lse = lsm;                          // [T]
    float* acc = lse + T;                      // [CTC_NW][C]
    int* lab = (int*)(acc + CTC_NW * C);       // [SP]
    float* logy = TLDS ? (float*)(lab + SP) : ws + (size_t)n * 3 * T * SP;     // [T][SP] each
    float* alpha = logy + (size_t)T * SP;
    float* beta = alpha + (size_t)T * SP;
    __shared__ float s_logp;
    __shared__ int s_cnt[2];

    const int L = label_len[n];
    const int Tn = min(input_len[n], T);
    const int S = 2 * L + 1;
    const size_t tstride = (size_t)N * C;
    const float* a_n = act + (size_t)n * C;
    float* g_n = grad ? grad + (size_t)n * C : nullptr;
    bf16_t* gb_n = grad_ntc ? grad_ntc + (size_t)n * T * C : nullptr;
    const bool want_grad = g_n || gb_n;

    const bool feasible = ctc_sample_setup(flat_labels, label_len, n, L, Tn, SP, blank, lab, s_cnt, 64 * CTC_NW);
    if (want_grad) ctc_zero_frames(g_n, gb_n, feasible ? Tn : 0, T, C, tstride, lane, wave, CTC_NW);
    if (!feasible) { if (tid == 0) costs[n] = 0.f; return; }

    // phase 1: softmax denominators
    for (int t = wave; t < Tn; t += CTC_NW) {
        const float l = ctc_row_lse(a_n + t * tstride, C, lane);
        if (lane == 0) lse[t] = l;
    }
    __syncthreads();
    // phase 2: logy table, every slot of every owned frame (-inf beyond S)
    for (int i = tid; i < Tn * SP; i += 64 * CTC_NW) {
        const int t = i / SP, j = i & (SP - 1);
        const int s = (j & 63) * VT + (j >> 6);
        logy[i] = (s < S) ? a_n[t * tstride + lab[s]] - lse[t] : NEG_INF;
    }
    __syncthreads();
    // phase 3
    ctc_long_recursions<VT>(lane, wave, S, Tn, blank, want_grad, lab, logy, alpha, beta, &s_logp, costs + n);
    __syncthreads();
    if (!want_grad) return;
    // phase 4: gradient rows
    const float logp = s_logp;
    float* wacc = acc + wave * C;
    for (int t = wave; t < Tn; t += CTC_NW) {
        for (int k = lane; k < C; k += 64) wacc[k] = 0.f;
        const size_t base = (size_t)t * SP + lane;
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const int s = lane * VT + v;
            if (s < S) ctc_posterior_add(&wacc[lab[s]], alpha[base + v * 64], beta[base + v * 64], logy[base + v * 64], logp);
        }
        ctc_grad_row(a_n + t * tstride, lse[t], wacc, g_n, gb_n, t, tstride, C, lane, scale);
    }
}

constexpr size_t CTC_LONG_LDS_MAX = 128 * 1024;
constexpr int CTC_LONG_MAX_LABEL = 255;
static inline int ctc_long_vt(int max_label_len) { const int s = smax_for(max_label_len); return s <= 128 ? 2 : s <= 256 ? 4 : 8; }
// LDS without the tables: lse[T], acc[CTC_NW][C], lab[SP]
static size_t ctc_long_lds_base(int C, int T, int SP) { return ((size_t)T + (size_t)CTC_NW * C + SP) * sizeof(float); }
static size_t ctc_long_table_bytes(int T, int SP) { return (size_t)3 * T * SP * sizeof(float); }
// 0: not covered; 1: tables in LDS; 2: tables in the workspace.  Arithmetic only.
extern "C" int ocr_ctc_long_placement(int alphabet_size, int max_time, int max_label_len) {
    if (alphabet_size <= 0 || max_time <= 0 || max_label_len <= 0 || max_label_len > CTC_LONG_MAX_LABEL) return 0;
    const int SP = 64 * ctc_long_vt(max_label_len);
    const size_t base = ctc_long_lds_base(alphabet_size, max_time, SP);
    if (base > CTC_LONG_LDS_MAX) return 0;
    return base + ctc_long_table_bytes(max_time, SP) <= CTC_LONG_LDS_MAX ? 1 : 2;
}
template <int VT, bool TLDS>
static int ctc_long_launch(const float* act, float* grad, bf16_t* gb, float scale, const int* labels, const int* ll, const int* il, int C, int N,
                           int T, int blank, float* costs, float* ws, size_t lds, hipStream_t stream, bool launch) {
    if (ocr_allow_lds<ctc_long_kernel<VT, TLDS>>((int)CTC_LONG_LDS_MAX) != hipSuccess) return OCR_ERR_INVALID;
    if (!launch) return OCR_OK;
    ctc_long_kernel<VT, TLDS><<<N, 64 * CTC_NW, lds, stream>>>(act, grad, labels, ll, il, T, N, C, blank, costs, gb, scale, ws);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
static int ctc_long_dispatch(const float* act, float* grad, bf16_t* gb, float scale, const int* labels, const int* ll, const int* il, int C, int N,
                             int T, int max_label_len, int blank, float* costs, float* ws, hipStream_t stream, bool launch) {
    const int place = ocr_ctc_long_placement(C, T, max_label_len);
    if (!place) return OCR_ERR_INVALID;
    const int VT = ctc_long_vt(max_label_len);
    const size_t lds = ctc_long_lds_base(C, T, 64 * VT) + (place == 1 ? ctc_long_table_bytes(T, 64 * VT) : 0);
#define CTC_LONG_CASE(V, B) return ctc_long_launch<V, B>(act, grad, gb, scale, labels, ll, il, C, N, T, blank, costs, ws, lds, stream, launch)
    if (place == 1) { if (VT == 2) CTC_LONG_CASE(2, true); if (VT == 4) CTC_LONG_CASE(4, true); CTC_LONG_CASE(8, true); }
    if (VT == 2) CTC_LONG_CASE(2, false);
    if (VT == 4) CTC_LONG_CASE(4, false);
    CTC_LONG_CASE(8, false);
#undef CTC_LONG_CASE
}
extern "C" int ocr_ctc_long_supported(int alphabet_size, int max_time, int max_label_len) {
    return ctc_long_dispatch(nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, alphabet_size, 1, max_time, max_label_len, 0, nullptr,
                             nullptr, nullptr, false) == OCR_OK;
}
extern "C" int ocr_ctc_long_workspace_size(int alphabet_size, int max_label_len, int max_time, int minibatch, size_t* bytes) {
    if (!bytes || minibatch <= 0) return OCR_ERR_INVALID;
    const int place = ocr_ctc_long_placement(alphabet_size, max_time, max_label_len);
    if (!place) return OCR_ERR_INVALID;
    *bytes = place == 1 ? 0 : ctc_align256((size_t)minibatch * ctc_long_table_bytes(max_time, 64 * ctc_long_vt(max_label_len)));
    return OCR_OK;
}
extern "C" int ocr_ctc_loss_long(const float* activations, float* gradients, void* grad_ntc_bf16, float scale, const int* flat_labels,
                                 const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch, int max_time,
                                 int max_label_len, int blank_label, float* costs, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!ctc_loss_args_ok(activations, flat_labels, label_lengths, input_lengths, costs, alphabet_size, minibatch, max_time, max_label_len, blank_label))
        return OCR_ERR_INVALID;
    size_t need = 0;
    if (ocr_ctc_long_workspace_size(alphabet_size, max_label_len, max_time, minibatch, &need) != OCR_OK) return OCR_ERR_INVALID;
    if (need && (!workspace || workspace_bytes < need)) return OCR_ERR_INVALID;
    return ctc_long_dispatch(activations, gradients, (bf16_t*)grad_ntc_bf16, scale, flat_labels, label_lengths, input_lengths, alphabet_size,
                             minibatch, max_time, max_label_len, blank_label, costs, (float*)workspace, (hipStream_t)stream_, true);
}

// ------------------------------------------------------------------------------------------------------------------
// Wide alphabets (1 <= C <= 16384, 1 <= L <= 255): the class-wide work on the whole chip, the recursion on one workgroup per sample.
// ctc_fast_kernel and ctc_long_kernel keep acc[CTC_NW][C] in LDS and give a sample's whole softmax to one workgroup; here that work is two launches, ordered by
// the stream (no workgroup waits on another):
//   ctc_wide_rows_kernel     one workgroup per logit row (t, n).  The row is read once into registers (16 elements a thread); the workgroup
//                            reduces max and sum, writes softmax (* scale) to the bf16 [N][T][C] and / or f32 [T][N][C] gradient as if no
//                            label were there, and gathers logy[t][s] = a[lab[s]] - lse into the sample's table in the workspace, in
//                            ctc_long_kernel's [T][SP] layout.  Rows with t >= Tn and all rows of an infeasible sample are zeros.
//   ctc_wide_samples_kernel  one workgroup per sample: ctc_long_recursions on that table (alpha, beta beside it in the workspace), then the
//                            fix-up: per frame the slot posteriors are summed per class through the class's first slot (canon[s]; every blank
//                            slot is slot 0), so a wave's accumulator is [SP] floats, not [C], and each first slot overwrites its one gradient
//                            element with exp(logy) - sum, rounded once from float32.
// Every workgroup of both kernels derives its sample's label offset, extended label and feasibility itself (ctc_sample_setup).
// ------------------------------------------------------------------------------------------------------------------
constexpr int CTC_WIDE_MAX_C = 16384;
constexpr int CTC_WIDE_PER = 16;        // row elements a thread of the rows kernel keeps: 256 threads cover C <= 4096, 512 cover 8192, 1024 cover 16384

// VEC consecutive row elements per load / store: 8 (C % 8 == 0: 2 x 16-byte loads, 16-byte bf16 store), 4 (C % 4 == 0) or 1 (any C)
template <int NT, int VEC>
__global__ __launch_bounds__(NT) void ctc_wide_rows_kernel(
    const float* __restrict__ act, float* __restrict__ grad, bf16_t* __restrict__ grad_ntc, float scale, const int* __restrict__ flat_labels,
    const int* __restrict__ label_len, const int* __restrict__ input_len, int T, int N, int C, int blank, int VT, float* __restrict__ ws) {
    constexpr int NW = NT / 64, NCH = CTC_WIDE_PER / VEC;
    const int r = blockIdx.x, t = r / N, n = r - t * N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int SP = 64 * VT;
    __shared__ int lab[64 * 8];
    __shared__ int s_cnt[2];
    __shared__ float s_max[NW], s_sum[NW];

    const int L = label_len[n];
    const int Tn = min(input_len[n], T);
    const int S = 2 * L + 1;
    const float* row = act + (size_t)r * C;
    float* grow = grad ? grad + (size_t)r * C : nullptr;
    bf16_t* gbrow = grad_ntc ? grad_ntc + ((size_t)n * T + t) * C : nullptr;

    // the row, in flight while the label is read
    float v[CTC_WIDE_PER];
    ctc_load_row<NT, VEC>(row, C, tid, t < Tn, v);
    const bool live = ctc_sample_setup(flat_labels, label_len, n, L, Tn, SP, blank, lab, s_cnt, NT) && t < Tn;

    float inv = 0.f, lse = 0.f;
    if (live) {
        const float m = ctc_row_max<NW>(v, s_max, lane, wave);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < CTC_WIDE_PER; ++j) { v[j] = __expf(v[j] - m); sum += v[j]; }      // (elements past C: exp(-inf) = 0; kept for the store below)
        sum = ctc_row_sum<NW>(sum, s_sum, lane, wave);
        inv = 1.f / sum;
        lse = m + logf(sum);
        // logy of every slot of this frame (-inf beyond S); the gathered logits are L2 hits of the loads above
        float* logy = ws + ((size_t)n * 3 * T + t) * SP;
        for (int j = tid; j < SP; j += NT) {
            const int s = (j & 63) * VT + (j >> 6);
            logy[j] = (s < S) ? row[lab[s]] - lse : NEG_INF;
        }
    }
    // softmax * scale (live) or zeros
    if (!grow && !gbrow) return;
    const float gs = inv * scale;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int k = (i * NT + tid) * VEC;
        if (k >= C) continue;
        const float* e = v + i * VEC;
        if constexpr (VEC == 1) {
            if (grow) grow[k] = live ? e[0] * inv : 0.f;
            if (gbrow) gbrow[k] = live ? f2bf(e[0] * gs) : (bf16_t)0;
        } else {
            if (grow) {
#pragma unroll
                for (int q = 0; q < VEC / 4; ++q) {
                    f32x4 o = {e[4 * q] * inv, e[4 * q + 1] * inv, e[4 * q + 2] * inv, e[4 * q + 3] * inv};
                    if (!live) o = (f32x4){0.f, 0.f, 0.f, 0.f};
                    *(f32x4*)(grow + k + 4 * q) = o;
                }
            }
            if (gbrow) {
                uint32_t pk[VEC / 2];
#pragma unroll
                for (int q = 0; q < VEC / 2; ++q) pk[q] = live ? pack_bf2(e[2 * q] * gs, e[2 * q + 1] * gs) : 0u;
                if constexpr (VEC == 8) *(u32x4*)(gbrow + k) = (u32x4){pk[0], pk[1], pk[2], pk[3]};
                else *(u32x2*)(gbrow + k) = (u32x2){pk[0], pk[1]};
            }
        }
    }
}

template <int VT>
__global__ __launch_bounds__(64 * CTC_NW) void ctc_wide_samples_kernel(
    float* __restrict__ grad, bf16_t* __restrict__ grad_ntc, float scale, const int* __restrict__ flat_labels, const int* __restrict__ label_len,
    const int* __restrict__ input_len, int T, int N, int C, int blank, float* __restrict__ costs, float* ws) {
    constexpr int SP = 64 * VT;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float acc[CTC_NW][SP];      // per-wave posterior sums, by first slot of the class
    __shared__ int lab[SP], canon[SP];
    __shared__ int s_cnt[2];
    __shared__ float s_logp;

    const int L = label_len[n];
    const int Tn = min(input_len[n], T);
    const int S = 2 * L + 1;
    const size_t tstride = (size_t)N * C;
    float* g_n = grad ? grad + (size_t)n * C : nullptr;
    bf16_t* gb_n = grad_ntc ? grad_ntc + (size_t)n * T * C : nullptr;
    const bool want_grad = g_n || gb_n;
    float* logy = ws + (size_t)n * 3 * T * SP;        // filled by ctc_wide_rows_kernel; alpha and beta are written and read by this workgroup only
    float* alpha = logy + (size_t)T * SP;
    float* beta = alpha + (size_t)T * SP;

    if (!ctc_sample_setup(flat_labels, label_len, n, L, Tn, SP, blank, lab, s_cnt, 64 * CTC_NW)) { if (tid == 0) costs[n] = 0.f; return; }
    // canon[s]: the first slot that holds slot s's class
    for (int s = tid; s < SP; s += 64 * CTC_NW) {
        int c = s;
        const int k = lab[s];
        for (int q = 0; q < s; ++q) if (lab[q] == k) { c = q; break; }
        canon[s] = c;
    }
    ctc_long_recursions<VT>(lane, wave, S, Tn, blank, want_grad, lab, logy, alpha, beta, &s_logp, costs + n);
    __syncthreads();
    if (!want_grad) return;
    // fix-up: the at most S gradient elements of each frame that are not plain softmax
    const float logp = s_logp;
    float* wacc = acc[wave];
    for (int t = wave; t < Tn; t += CTC_NW) {
        const size_t base = (size_t)t * SP + lane;
        float ly[VT];
#pragma unroll
        for (int v = 0; v < VT; ++v) wacc[v * 64 + lane] = 0.f;
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const int s = lane * VT + v;
            ly[v] = logy[base + v * 64];
            if (s < S) ctc_posterior_add(&wacc[canon[s]], alpha[base + v * 64], beta[base + v * 64], ly[v], logp);
        }
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const int s = lane * VT + v;
            if (s < S && canon[s] == s) {
                const float g = expf(ly[v]) - wacc[s];
                const int k = lab[s];
                ctc_grad_store(g, g_n, gb_n, t, k, tstride, C, scale);
            }
        }
    }
}

extern "C" int ocr_ctc_wide_supported(int alphabet_size, int max_time, int max_label_len) {
    return alphabet_size > 0 && alphabet_size <= CTC_WIDE_MAX_C && max_time > 0 && max_label_len >= 1 && max_label_len <= CTC_LONG_MAX_LABEL;
}
// the logy, alpha and beta tables of every sample
extern "C" int ocr_ctc_wide_workspace_size(int alphabet_size, int max_label_len, int max_time, int minibatch, size_t* bytes) {
    if (!bytes || minibatch <= 0 || !ocr_ctc_wide_supported(alphabet_size, max_time, max_label_len)) return OCR_ERR_INVALID;
    *bytes = ctc_align256((size_t)minibatch * ctc_long_table_bytes(max_time, 64 * ctc_long_vt(max_label_len)));
    return OCR_OK;
}
template <int NT, int VEC>
static void ctc_wide_rows_launch(const float* act, float* grad, bf16_t* gb, float scale, const int* labels, const int* ll, const int* il, int C, int N,
                                 int T, int blank, int VT, float* ws, hipStream_t stream) {
    ctc_wide_rows_kernel<NT, VEC><<<N * T, NT, 0, stream>>>(act, grad, gb, scale, labels, ll, il, T, N, C, blank, VT, ws);
}
extern "C" int ocr_ctc_loss_wide(const float* activations, float* gradients, void* grad_ntc_bf16, float scale, const int* flat_labels,
                                 const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch, int max_time,
                                 int max_label_len, int blank_label, float* costs, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!workspace || !ctc_loss_args_ok(activations, flat_labels, label_lengths, input_lengths, costs, alphabet_size, minibatch, max_time, max_label_len,
                                        blank_label) ||
        (long)minibatch * max_time > 0x7fffffffL)
        return OCR_ERR_INVALID;
    size_t need = 0;
    if (ocr_ctc_wide_workspace_size(alphabet_size, max_label_len, max_time, minibatch, &need) != OCR_OK || workspace_bytes < need) return OCR_ERR_INVALID;
    const int C = alphabet_size, N = minibatch, T = max_time, VT = ctc_long_vt(max_label_len);
    bf16_t* gb = (bf16_t*)grad_ntc_bf16;
    float* ws = (float*)workspace;
    const bool al16 = (((uintptr_t)activations | (uintptr_t)gradients | (uintptr_t)gb) & 15) == 0;
    const int VEC = (al16 && C % 8 == 0) ? 8 : (al16 && C % 4 == 0) ? 4 : 1;
#define CTC_WIDE_ROWS(NT, V) ctc_wide_rows_launch<NT, V>(activations, gradients, gb, scale, flat_labels, label_lengths, input_lengths, C, N, T, blank_label, VT, ws, stream)
    // the smallest workgroup whose threads hold the row: more workgroups per CU hide each one's barriers and label reads
    if (C <= 256 * CTC_WIDE_PER) { if (VEC == 8) CTC_WIDE_ROWS(256, 8); else if (VEC == 4) CTC_WIDE_ROWS(256, 4); else CTC_WIDE_ROWS(256, 1); }
    else if (C <= 512 * CTC_WIDE_PER) { if (VEC == 8) CTC_WIDE_ROWS(512, 8); else if (VEC == 4) CTC_WIDE_ROWS(512, 4); else CTC_WIDE_ROWS(512, 1); }
    else { if (VEC == 8) CTC_WIDE_ROWS(1024, 8); else if (VEC == 4) CTC_WIDE_ROWS(1024, 4); else CTC_WIDE_ROWS(1024, 1); }
#undef CTC_WIDE_ROWS
    OCR_CHECK_LAUNCH();
#define CTC_WIDE_SAMPLES(V) ctc_wide_samples_kernel<V><<<N, 64 * CTC_NW, 0, stream>>>(gradients, gb, scale, flat_labels, label_lengths, input_lengths, T, N, C, blank_label, costs, ws)
    if (VT == 2) CTC_WIDE_SAMPLES(2); else if (VT == 4) CTC_WIDE_SAMPLES(4); else CTC_WIDE_SAMPLES(8);
#undef CTC_WIDE_SAMPLES
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
