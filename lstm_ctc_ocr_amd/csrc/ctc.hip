// CTC loss + gradient and greedy decode for gfx950: one 64-lane wavefront per sample.
//
// Replaces the un-vendored baidu warp-ctc kernels the reference reaches through
// `warpctc_tensorflow.ctc(...)` (reference lib/networks/network.py:653-654) and the best-path
// part of the decode at network.py:656-657 / lib/lstm/test.py:30-31.
//
// Semantics (SURVEY.md Appendix A "CTC (warp-ctc)"):
//   y = softmax_C(act[t,n,:]);  l' = [b,l1,b,...,lL,b], S = 2L+1, b = blank_label
//   cost_n = -log p(l|x);  d cost/d act[t,n,k] = y[t,n,k] - sum_{s: l'_s = k} gamma_t(s)
//   for t < input_length, 0 beyond;  infeasible (L + repeats > T) => cost 0, grad 0.
//
// Mapping: lane s (+64*v) owns extended-label slot s; the alpha row lives in LDS so the
// s-1 / s-2 neighbours are one ds_read away; a single wave per workgroup means the
// step-to-step barrier is free. alpha[T][S] is parked in a caller-owned workspace in HBM
// (L2-resident at these sizes); beta is consumed on the fly while the gradient row is
// produced with all 64 lanes striding the class axis (one coalesced 256-B row at C = 64).
#include "common.h"
#include <math.h>

// (NEG_INF and the DPP wave shifts wave_shr1 / wave_shl1 are in common.h, shared with ctc_score.hip)
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

// VT = extended-label slots per lane (S <= 64*VT).
template <int VT>
__global__ __launch_bounds__(64) void ctc_loss_grad_kernel(
    const float* __restrict__ act,      // [T, N, C] unnormalised
    float* __restrict__ grad,           // [T, N, C] or nullptr
    const int* __restrict__ flat_labels,
    const int* __restrict__ label_off,  // [N] exclusive prefix sum of label_lengths
    const int* __restrict__ label_len,  // [N]
    const int* __restrict__ input_len,  // [N]
    int T, int N, int C, int blank,
    float* __restrict__ costs,          // [N]
    float* __restrict__ ws,             // workspace: per sample T*(SMAX+1) floats
    int SMAX) {
    const int n = blockIdx.x;
    const int lane = threadIdx.x;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // LDS carve-up: row[2][SMAX+2] (ping-pong alpha/beta rows, 2 guard slots in front),
    //               acc[C] (posterior per class), lab[SMAX] (extended labels as int)
    float* rowbuf = smem;                              // 2*(SMAX+2)
    float* acc = rowbuf + 2 * (SMAX + 2);              // C
    int* lab = (int*)(acc + C);                        // SMAX

    const int L = label_len[n];
    const int Tn = min(input_len[n], T);
    const int S = 2 * L + 1;
    const int* labels = flat_labels + label_off[n];
    float* alpha_ws = ws + (size_t)n * T * (SMAX + 1);   // alpha[t][s]; slot SMAX of row t = lse[t]
    const size_t tstride = (size_t)N * C;
    const float* a_n = act + (size_t)n * C;
    float* g_n = grad ? grad + (size_t)n * C : nullptr;

    // zero-fill the gradient of frames this sample does not own (t >= Tn)
    if (g_n) {
        for (int t = Tn; t < T; ++t)
            for (int k = lane; k < C; k += 64) g_n[t * tstride + k] = 0.f;
    }

    // extended labels + repeat count
    int repeats = 0;
    for (int s = lane; s < S; s += 64) {
        int v = (s & 1) ? labels[s >> 1] : blank;
        lab[s] = v;
        if ((s & 1) && s >= 3 && labels[s >> 1] == labels[(s >> 1) - 1]) repeats++;
    }
    repeats = (int)wave_sum((float)repeats);
    __syncthreads();

    if (L + repeats > Tn || Tn <= 0) {   // infeasible alignment: warp-ctc reports cost 0, grad 0
        if (lane == 0) costs[n] = 0.f;
        if (g_n)
            for (int t = 0; t < Tn; ++t)
                for (int k = lane; k < C; k += 64) g_n[t * tstride + k] = 0.f;
        return;
    }

    // ---- pass 1: log-sum-exp of every frame (softmax denominator), parked at alpha_ws[t][SMAX]
    for (int t = 0; t < Tn; ++t) {
        const float* row = a_n + t * tstride;
        float m = NEG_INF;
        for (int k = lane; k < C; k += 64) m = fmaxf(m, row[k]);
        m = wave_max(m);
        float sum = 0.f;
        for (int k = lane; k < C; k += 64) sum += expf(row[k] - m);
        sum = wave_sum(sum);
        if (lane == 0) alpha_ws[(size_t)t * (SMAX + 1) + SMAX] = m + logf(sum);
    }
    __syncthreads();

    // per-slot constants
    int my_lab[VT];
    bool skip_fwd[VT], skip_bwd[VT];
#pragma unroll
    for (int v = 0; v < VT; ++v) {
        int s = lane + 64 * v;
        my_lab[v] = (s < S) ? lab[s] : blank;
        skip_fwd[v] = (s < S) && (s >= 2) && (my_lab[v] != blank) && (my_lab[v] != lab[s - 2]);
        skip_bwd[v] = (s + 2 < S) && (lab[s + 2] != blank) && (lab[s + 2] != my_lab[v]);
    }

    // ---- pass 2: alpha recursion, rows kept in the workspace
    float* cur = rowbuf + 2;                 // cur[-1], cur[-2] are guard slots (= -inf)
    float* nxt = rowbuf + (SMAX + 2) + 2;
    if (lane < 2) { cur[-1 - lane] = NEG_INF; nxt[-1 - lane] = NEG_INF; }
    {
        float lse0 = alpha_ws[SMAX];
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            int s = lane + 64 * v;
            if (s < S) {
                float a0 = (s < 2) ? (a_n[my_lab[v]] - lse0) : NEG_INF;
                cur[s] = a0;
                alpha_ws[s] = a0;
            }
        }
    }
    __syncthreads();
    for (int t = 1; t < Tn; ++t) {
        const float* row = a_n + t * tstride;
        float lse_t = alpha_ws[(size_t)t * (SMAX + 1) + SMAX];
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            int s = lane + 64 * v;
            if (s < S) {
                float p0 = cur[s], p1 = cur[s - 1];
                float p2 = skip_fwd[v] ? cur[s - 2] : NEG_INF;
                float a = lse3(p0, p1, p2);
                if (a != NEG_INF) a += row[my_lab[v]] - lse_t;
                nxt[s] = a;
                alpha_ws[(size_t)t * (SMAX + 1) + s] = a;
            }
        }
        __syncthreads();
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    // log p(l|x)
    float logp;
    {
        float e1 = cur[S - 1];
        float e2 = (S >= 2) ? cur[S - 2] : NEG_INF;
        logp = lse2(e1, e2);
    }
    if (lane == 0) costs[n] = -logp;
    if (!g_n) return;
    __syncthreads();

    // ---- pass 3: beta recursion fused with the gradient rows (t = Tn-1 .. 0)
    // rows here carry 2 guard slots BEHIND the data (s = S, S+1) instead of in front
    float* bcur = rowbuf;
    float* bnxt = rowbuf + (SMAX + 2);
    for (int t = Tn - 1; t >= 0; --t) {
        const float* row = a_n + t * tstride;
        float lse_t = alpha_ws[(size_t)t * (SMAX + 1) + SMAX];
        for (int k = lane; k < C; k += 64) acc[k] = 0.f;
        __syncthreads();
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            int s = lane + 64 * v;
            if (s < S) {
                float ly = row[my_lab[v]] - lse_t;
                float b;
                if (t == Tn - 1) {
                    b = (s >= S - 2) ? ly : NEG_INF;
                } else {
                    float q0 = bcur[s];
                    float q1 = (s + 1 < S) ? bcur[s + 1] : NEG_INF;
                    float q2 = skip_bwd[v] ? bcur[s + 2] : NEG_INF;
                    b = lse3(q0, q1, q2);
                    if (b != NEG_INF) b += ly;
                }
                bnxt[s] = b;
                float al = alpha_ws[(size_t)t * (SMAX + 1) + s];
                if (al != NEG_INF && b != NEG_INF) {
                    float gamma = expf(al + b - ly - logp);   // posterior of (t, s), <= 1
                    atomicAdd(&acc[my_lab[v]], gamma);
                }
            }
        }
        __syncthreads();
        float* grow = g_n + t * tstride;
        for (int k = lane; k < C; k += 64) grow[k] = expf(row[k] - lse_t) - acc[k];
        float* tmp = bcur; bcur = bnxt; bnxt = tmp;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Fast path (S = 2L+1 <= 64 and 3*T*S floats fit in LDS — every configuration of the reference): 4 waves per sample.
//   phase 1  all waves: softmax denominators of their frames (t = wave, wave+4, ...)
//   phase 2  all threads: logy[t][s] = act[t][l'_s] - lse[t] gathered into LDS — the recursion below never waits on HBM/L2
//   phase 3  wave 0 runs the alpha recursion, wave 1 the beta recursion CONCURRENTLY; the row lives in registers and the
//            s-1 / s-2 (s+1 / s+2) neighbours come from wave shuffles, so a step is ~60 VALU cycles with no barrier
//   phase 4  all waves: gradient rows of their frames (posterior per class via LDS float atomics, coalesced row store)
// The first version did all of this in one wave with a barrier and an L2 round trip per step: 3 x 63 serial steps,
// ~0.8 us each (152 us at T = 63).
// ------------------------------------------------------------------------------------------------------------------
__device__ long long* g_ctc_dbg = nullptr;
constexpr int CTC_NW = 16;        // waves per sample: the frame-parallel phases (log-sum-exp rows, gradient rows) are latency chains per
                                  // row (cross-lane reductions, LDS atomics): 16 waves x 4 rows instead of 4 x 16 rows
__global__ __launch_bounds__(64 * CTC_NW) void ctc_fast_kernel(
    const float* __restrict__ act, float* __restrict__ grad, const int* __restrict__ flat_labels,
    const int* __restrict__ label_off, const int* __restrict__ label_len, const int* __restrict__ input_len,
    int T, int N, int C, int blank, float* __restrict__ costs, int SMAX,
    bf16_t* __restrict__ grad_ntc /* optional: bf16 [N][T][C] = scale * gradient (the layout/dtype the backward GEMMs read) */,
    float scale) {
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    float* lse = fsm;                          // [T]
    float* logy = lse + T;                     // [T][SMAX]
    float* alpha = logy + T * SMAX;            // [T][SMAX]
    float* beta = alpha + T * SMAX;            // [T][SMAX]
    float* acc = beta + T * SMAX;              // [CTC_NW][C]   per-wave posterior accumulators
    int* lab = (int*)(acc + CTC_NW * C);       // [SMAX]
    __shared__ float s_logp;
    __shared__ int s_repeats, s_off;

    const int L = label_len[n];
    const int Tn = min(input_len[n], T);
    const int S = 2 * L + 1;
    const size_t tstride = (size_t)N * C;
    const float* a_n = act + (size_t)n * C;
    float* g_n = grad ? grad + (size_t)n * C : nullptr;
    bf16_t* gb_n = grad_ntc ? grad_ntc + (size_t)n * T * C : nullptr;
    const bool want_grad = g_n || gb_n;

    if (tid == 0) { s_repeats = 0; s_off = 0; }
    __syncthreads();
    if (label_off == nullptr) {            // exclusive prefix sum of the label lengths, done here instead of a scan launch
        int part = 0;
        for (int i = tid; i < n; i += 64 * CTC_NW) part += label_len[i];
        if (part) atomicAdd(&s_off, part);
        __syncthreads();
    }
    const int* labels = flat_labels + (label_off ? label_off[n] : s_off);
    int rep = 0;
    for (int s = tid; s < S; s += 64 * CTC_NW) {
        lab[s] = (s & 1) ? labels[s >> 1] : blank;
        if ((s & 1) && s >= 3 && labels[s >> 1] == labels[(s >> 1) - 1]) rep++;
    }
    if (rep) atomicAdd(&s_repeats, rep);
    __syncthreads();
    const bool feasible = (Tn > 0) && (L + s_repeats <= Tn);
    if (want_grad) {    // frames this sample does not own (and everything when infeasible): zero gradient
        const int t0 = feasible ? Tn : 0;
        for (int t = t0 + wave; t < T; t += CTC_NW)
            for (int k = lane; k < C; k += 64) {
                if (g_n) g_n[t * tstride + k] = 0.f;
                if (gb_n) gb_n[(size_t)t * C + k] = 0;
            }
    }
    if (!feasible) { if (tid == 0) costs[n] = 0.f; return; }
#define CSTAMP(k) do { if (g_ctc_dbg && n == 0 && tid == 0) g_ctc_dbg[k] = wall_clock64(); } while (0)
    CSTAMP(0);

    // phase 1.  A wave owns frames wave, wave+16, ...; when they fit (T <= 64, C <= 128) ALL its activation rows are loaded
    // first — independent loads, one memory round trip — and stay in registers for phase 4.  (Row after row, each frame paid
    // a dependent global-load latency: 12 us of the 41 us kernel here, 7.5 more in phase 4.)
    constexpr int MAXR = 4, MAXK = 2;
    const bool cached = (T <= CTC_NW * MAXR) && (C <= 64 * MAXK);
    float rowv[MAXR][MAXK];
    if (cached) {
#pragma unroll
        for (int i = 0; i < MAXR; ++i)
#pragma unroll
            for (int j = 0; j < MAXK; ++j) {
                const int t = wave + CTC_NW * i, k = lane + 64 * j;
                rowv[i][j] = (t < Tn && k < C) ? a_n[t * tstride + k] : NEG_INF;
            }
#pragma unroll
        for (int i = 0; i < MAXR; ++i) {
            const int t = wave + CTC_NW * i;
            float m = fmaxf(rowv[i][0], rowv[i][1]);
            m = wave_max(m);
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < MAXK; ++j) sum += (rowv[i][j] == NEG_INF) ? 0.f : expf(rowv[i][j] - m);
            sum = wave_sum(sum);
            if (lane == 0 && t < Tn) lse[t] = m + logf(sum);
        }
    } else
    for (int t = wave; t < Tn; t += CTC_NW) {
        const float* row = a_n + t * tstride;
        float m = NEG_INF;
        for (int k = lane; k < C; k += 64) m = fmaxf(m, row[k]);
        m = wave_max(m);
        float sum = 0.f;
        for (int k = lane; k < C; k += 64) sum += expf(row[k] - m);
        sum = wave_sum(sum);
        if (lane == 0) lse[t] = m + logf(sum);
    }
    __syncthreads();
    CSTAMP(1);
    // phase 2
    for (int i = tid; i < Tn * S; i += 64 * CTC_NW) {
        const int t = i / S, s = i - t * S;
        logy[t * SMAX + s] = a_n[t * tstride + lab[s]] - lse[t];
    }
    __syncthreads();
    CSTAMP(2);
    // phase 3
    if (wave == 0) {
        const int s = lane;
        const bool in = s < S;
        const int my = in ? lab[s] : blank;
        const bool skip = in && s >= 2 && my != blank && my != lab[s - 2];
        float a = (in && s < 2) ? logy[s] : NEG_INF;
        if (in) alpha[s] = a;
        for (int t = 1; t < Tn; ++t) {
            float p1 = wave_shr1(a, NEG_INF), p2 = wave_shr1(p1, NEG_INF);
            if (!skip) p2 = NEG_INF;
            float v = lse3_fast(a, p1, p2);
            if (v != NEG_INF && in) v += logy[t * SMAX + s]; else if (!in) v = NEG_INF;
            a = v;
            if (in) alpha[t * SMAX + s] = a;
        }
        float e1 = __shfl(a, S - 1, 64);
        float e2 = (S >= 2) ? __shfl(a, S - 2, 64) : NEG_INF;
        if (lane == 0) { s_logp = lse2(e1, e2); costs[n] = -s_logp; }
    } else if (wave == 1 && want_grad) {
        const int s = lane;
        const bool in = s < S;
        const int my = in ? lab[s] : blank;
        const bool skip = (s + 2 < S) && lab[s + 2] != blank && lab[s + 2] != my;
        float b = (in && s >= S - 2) ? logy[(Tn - 1) * SMAX + s] : NEG_INF;
        if (in) beta[(Tn - 1) * SMAX + s] = b;
        for (int t = Tn - 2; t >= 0; --t) {
            float q1 = wave_shl1(b, NEG_INF), q2 = wave_shl1(q1, NEG_INF);
            if (s + 1 >= S) q1 = NEG_INF;
            if (!skip) q2 = NEG_INF;
            float v = lse3_fast(b, q1, q2);
            if (v != NEG_INF && in) v += logy[t * SMAX + s]; else if (!in) v = NEG_INF;
            b = v;
            if (in) beta[t * SMAX + s] = b;
        }
    }
    __syncthreads();
    CSTAMP(3);
    if (!want_grad) return;
    // phase 4
    const float logp = s_logp;
    float* wacc = acc + wave * C;
    if (cached) {
#pragma unroll
        for (int i = 0; i < MAXR; ++i) {
            const int t = wave + CTC_NW * i;
            if (t >= Tn) break;                       // uniform per wave
            for (int k = lane; k < C; k += 64) wacc[k] = 0.f;
            if (lane < S) {
                const float al = alpha[t * SMAX + lane], be = beta[t * SMAX + lane];
                if (al != NEG_INF && be != NEG_INF) atomicAdd(&wacc[lab[lane]], expf(al + be - logy[t * SMAX + lane] - logp));
            }
            const float l = lse[t];
#pragma unroll
            for (int j = 0; j < MAXK; ++j) {
                const int k = lane + 64 * j;
                if (k < C) {
                    const float v = expf(rowv[i][j] - l) - wacc[k];
                    if (g_n) g_n[t * tstride + k] = v;
                    if (gb_n) gb_n[(size_t)t * C + k] = f2bf(v * scale);
                }
            }
        }
    } else
    for (int t = wave; t < Tn; t += CTC_NW) {
        for (int k = lane; k < C; k += 64) wacc[k] = 0.f;
        if (lane < S) {
            const float al = alpha[t * SMAX + lane], be = beta[t * SMAX + lane];
            if (al != NEG_INF && be != NEG_INF) atomicAdd(&wacc[lab[lane]], expf(al + be - logy[t * SMAX + lane] - logp));
        }
        const float* row = a_n + t * tstride;
        const float l = lse[t];
        for (int k = lane; k < C; k += 64) {
            const float v = expf(row[k] - l) - wacc[k];
            if (g_n) g_n[t * tstride + k] = v;
            if (gb_n) gb_n[(size_t)t * C + k] = f2bf(v * scale);
        }
    }
    CSTAMP(4);
}

// Greedy (best-path) decode: per frame argmax (lowest index wins ties, like numpy.argmax),
// collapse repeats, drop `blank`. Output is dense [N, T] padded with `pad_value`, plus lengths.
__global__ __launch_bounds__(64) void ctc_greedy_kernel(
    const float* __restrict__ act, const int* __restrict__ input_len, int T, int N, int C,
    int blank, int pad_value, int* __restrict__ out, int* __restrict__ out_len) {
    const int n = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ int am[64];
    const int Tn = min(input_len[n], T);
    int* o = out + (size_t)n * T;
    int prev = -1;
    int count = 0;
    for (int t0 = 0; t0 < Tn; t0 += 64) {
        int tcnt = min(64, Tn - t0);
        for (int tt = 0; tt < tcnt; ++tt) {
            const float* row = act + ((size_t)(t0 + tt) * N + n) * C;
            float bv = NEG_INF;
            int bi = 0x7fffffff;
            for (int k = lane; k < C; k += 64) {
                float v = row[k];
                if (v > bv) { bv = v; bi = k; }   // strict > keeps the lowest index per lane
            }
#pragma unroll
            for (int o2 = 32; o2 > 0; o2 >>= 1) {
                float ov = __shfl_xor(bv, o2, 64);
                int oi = __shfl_xor(bi, o2, 64);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) am[tt] = bi;
        }
        __syncthreads();
        int a = (lane < tcnt) ? am[lane] : blank;
        int before = __shfl_up(a, 1, 64);
        if (lane == 0) before = prev;
        bool keep = (lane < tcnt) && (a != blank) && (a != before);
        unsigned long long mask = __ballot(keep);
        int pos = __popcll(mask & ((1ull << lane) - 1ull));
        if (keep) o[count + pos] = a;
        count += __popcll(mask);
        prev = am[tcnt - 1];
        __syncthreads();
    }
    for (int j = count + lane; j < T; j += 64) o[j] = pad_value;
    if (lane == 0) out_len[n] = count;
}

__global__ void exclusive_scan_small(const int* __restrict__ in, int* __restrict__ out, int n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < n; ++i) { out[i] = s; s += in[i]; }
    }
}

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/ocr_hip.h)
// ------------------------------------------------------------------------------------------
static inline int smax_for(int max_label_len) { return 2 * max_label_len + 1; }
static int g_ctc_fast = 1;
extern "C" int ocr_set_ctc_engine(int fast) { g_ctc_fast = fast; return OCR_OK; }   // A/B + test knob: 0 = one-wave reference kernel

// the [T][S] tables of the fast kernel may need more than the 64 KiB of dynamic LDS a kernel gets by default (T = 79 of the
// variable-width workload: 65 KiB); the limit is raised once
constexpr size_t CTC_FAST_LDS_MAX = 128 * 1024;
static bool ctc_fast_allow_lds() {
    return ocr_allow_lds<ctc_fast_kernel>((int)CTC_FAST_LDS_MAX) == hipSuccess;
}

extern "C" int ocr_ctc_workspace_size(int max_label_len, int max_time, int minibatch,
                                      size_t* bytes) {
    if (!bytes || max_label_len < 0 || max_time <= 0 || minibatch <= 0) return OCR_ERR_INVALID;
    size_t smax = (size_t)smax_for(max_label_len);
    // alpha rows (+1 slot per row for the frame log-sum-exp) + label offsets
    *bytes = (size_t)minibatch * max_time * (smax + 1) * sizeof(float) +
             (size_t)minibatch * sizeof(int);
    *bytes = (*bytes + 255) & ~(size_t)255;
    return OCR_OK;
}

extern "C" int ocr_ctc_loss(const float* activations, float* gradients, const int* flat_labels,
                            const int* label_lengths, const int* input_lengths,
                            int alphabet_size, int minibatch, int max_time, int max_label_len,
                            int blank_label, float* costs, void* workspace, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!activations || !flat_labels || !label_lengths || !input_lengths || !costs || !workspace)
        return OCR_ERR_INVALID;
    if (alphabet_size <= 0 || minibatch <= 0 || max_time <= 0 || max_label_len < 0 ||
        blank_label < 0 || blank_label >= alphabet_size)
        return OCR_ERR_INVALID;
    const int SMAX = smax_for(max_label_len);
    if (SMAX > 256) return OCR_ERR_INVALID;   // 4 slots per lane is the largest instantiation
    float* ws = (float*)workspace;
    int* label_off = (int*)(ws + (size_t)minibatch * max_time * (SMAX + 1));
    exclusive_scan_small<<<1, 64, 0, stream>>>(label_lengths, label_off, minibatch);
    OCR_CHECK_LAUNCH();
    // fast path: S <= 64 and the three [T][S] tables fit in LDS
    {
        size_t flds = ((size_t)max_time * (1 + 3 * SMAX) + CTC_NW * (size_t)alphabet_size) * sizeof(float) + (size_t)SMAX * sizeof(int);
        flds = (flds + 15) & ~(size_t)15;
        if (SMAX <= 64 && flds <= CTC_FAST_LDS_MAX && g_ctc_fast && ctc_fast_allow_lds()) {
            ctc_fast_kernel<<<minibatch, 64 * CTC_NW, flds, stream>>>(activations, gradients, flat_labels, label_off, label_lengths,
                                                             input_lengths, max_time, minibatch, alphabet_size, blank_label, costs,
                                                             SMAX, nullptr, 1.0f);
            OCR_CHECK_LAUNCH();
            return OCR_OK;
        }
    }
    size_t lds = (size_t)(2 * (SMAX + 2) + alphabet_size) * sizeof(float) + (size_t)SMAX * sizeof(int);
    lds = (lds + 15) & ~(size_t)15;
    if (lds > 160 * 1024) return OCR_ERR_INVALID;
#define LAUNCH_CTC(VT)                                                                         \
    ctc_loss_grad_kernel<VT><<<minibatch, 64, lds, stream>>>(                                  \
        activations, gradients, flat_labels, label_off, label_lengths, input_lengths, max_time, \
        minibatch, alphabet_size, blank_label, costs, ws, SMAX)
    if (SMAX <= 64) LAUNCH_CTC(1);
    else if (SMAX <= 128) LAUNCH_CTC(2);
    else LAUNCH_CTC(4);
#undef LAUNCH_CTC
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}

static size_t ctc_fast_lds(int SMAX, int max_time, int alphabet_size) {
    size_t flds = ((size_t)max_time * (1 + 3 * SMAX) + CTC_NW * (size_t)alphabet_size) * sizeof(float) + (size_t)SMAX * sizeof(int);
    return (flds + 15) & ~(size_t)15;
}
// Training form: costs + the gradient ALREADY in the layout / dtype / scale the backward GEMMs consume
// (bf16 [N][T][C], multiplied by `scale` = 1/(batch*world)); label offsets are computed in-kernel.  One launch instead of
// scan + loss + transpose.  Covers S = 2L+1 <= 64 with the [T][S] tables in LDS; returns OCR_ERR_INVALID otherwise
// (callers then use ocr_ctc_loss + ocr_tnc_to_ntc_bf16).
extern "C" int ocr_ctc_debug(void* p) { long long* q = (long long*)p; return hipMemcpyToSymbol(HIP_SYMBOL(g_ctc_dbg), &q, sizeof(q)) == hipSuccess ? OCR_OK : OCR_ERR_MEMOPS; }
extern "C" int ocr_ctc_train_supported(int alphabet_size, int max_time, int max_label_len) {
    const int SMAX = smax_for(max_label_len);
    return SMAX <= 64 && ctc_fast_lds(SMAX, max_time, alphabet_size) <= CTC_FAST_LDS_MAX && ctc_fast_allow_lds();
}
extern "C" int ocr_ctc_loss_train(const float* activations, void* grad_ntc_bf16, float scale, const int* flat_labels,
                                  const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                                  int max_time, int max_label_len, int blank_label, float* costs, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!activations || !grad_ntc_bf16 || !flat_labels || !label_lengths || !input_lengths || !costs) return OCR_ERR_INVALID;
    if (alphabet_size <= 0 || minibatch <= 0 || max_time <= 0 || max_label_len < 0 || blank_label < 0 ||
        blank_label >= alphabet_size || !ocr_ctc_train_supported(alphabet_size, max_time, max_label_len))
        return OCR_ERR_INVALID;
    const int SMAX = smax_for(max_label_len);
    ctc_fast_kernel<<<minibatch, 64 * CTC_NW, ctc_fast_lds(SMAX, max_time, alphabet_size), stream>>>(
        activations, nullptr, flat_labels, nullptr, label_lengths, input_lengths, max_time, minibatch, alphabet_size, blank_label,
        costs, SMAX, (bf16_t*)grad_ntc_bf16, scale);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}

extern "C" int ocr_ctc_greedy_decode(const float* activations, const int* input_lengths,
                                     int alphabet_size, int minibatch, int max_time,
                                     int blank_label, int pad_value, int* decoded,
                                     int* decoded_lengths, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!activations || !input_lengths || !decoded || !decoded_lengths) return OCR_ERR_INVALID;
    if (alphabet_size <= 0 || minibatch <= 0 || max_time <= 0) return OCR_ERR_INVALID;
    ctc_greedy_kernel<<<minibatch, 64, 0, stream>>>(activations, input_lengths, max_time, minibatch,
                                                    alphabet_size, blank_label, pad_value, decoded,
                                                    decoded_lengths);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}

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
        float x1 = NEG_INF, x2 = NEG_INF;
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            if (v == ((S - 1) & (VT - 1))) x1 = a[v];
            if (S >= 2 && v == ((S - 2) & (VT - 1))) x2 = a[v];
        }
        const float e1 = __shfl(x1, (S - 1) / VT, 64);
        const float e2 = (S >= 2) ? __shfl(x2, (S - 2) / VT, 64) : NEG_INF;
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
    __shared__ int s_repeats, s_off;

    const int L = label_len[n];
    const int Tn = min(input_len[n], T);
    const int S = 2 * L + 1;
    const size_t tstride = (size_t)N * C;
    const float* a_n = act + (size_t)n * C;
    float* g_n = grad ? grad + (size_t)n * C : nullptr;
    bf16_t* gb_n = grad_ntc ? grad_ntc + (size_t)n * T * C : nullptr;
    const bool want_grad = g_n || gb_n;

    if (tid == 0) { s_repeats = 0; s_off = 0; }
    __syncthreads();
    {                                      // exclusive prefix sum of the label lengths
        int part = 0;
        for (int i = tid; i < n; i += 64 * CTC_NW) part += label_len[i];
        if (part) atomicAdd(&s_off, part);
        __syncthreads();
    }
    const int* labels = flat_labels + s_off;
    const bool fits = L >= 0 && S <= SP;   // a label longer than the declared capacity has no table: treated like an infeasible sample
    int rep = 0;
    for (int s = tid; s < SP; s += 64 * CTC_NW) {
        const bool in = fits && s < S;
        lab[s] = (in && (s & 1)) ? labels[s >> 1] : blank;
        if (in && (s & 1) && s >= 3 && labels[s >> 1] == labels[(s >> 1) - 1]) rep++;
    }
    if (rep) atomicAdd(&s_repeats, rep);
    __syncthreads();
    const bool feasible = fits && (Tn > 0) && (L + s_repeats <= Tn);
    if (want_grad) {    // frames this sample does not own (and everything when infeasible): zero gradient
        const int t0 = feasible ? Tn : 0;
        for (int t = t0 + wave; t < T; t += CTC_NW)
            for (int k = lane; k < C; k += 64) {
                if (g_n) g_n[t * tstride + k] = 0.f;
                if (gb_n) gb_n[(size_t)t * C + k] = 0;
            }
    }
    if (!feasible) { if (tid == 0) costs[n] = 0.f; return; }

    // phase 1: softmax denominators
    for (int t = wave; t < Tn; t += CTC_NW) {
        const float* row = a_n + t * tstride;
        float m = NEG_INF;
        for (int k = lane; k < C; k += 64) m = fmaxf(m, row[k]);
        m = wave_max(m);
        float sum = 0.f;
        for (int k = lane; k < C; k += 64) sum += expf(row[k] - m);
        sum = wave_sum(sum);
        if (lane == 0) lse[t] = m + logf(sum);
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
            if (s < S) {
                const float al = alpha[base + v * 64], be = beta[base + v * 64];
                if (al != NEG_INF && be != NEG_INF) atomicAdd(&wacc[lab[s]], expf(al + be - logy[base + v * 64] - logp));
            }
        }
        const float* row = a_n + t * tstride;
        const float l = lse[t];
        for (int k = lane; k < C; k += 64) {
            const float v = expf(row[k] - l) - wacc[k];
            if (g_n) g_n[t * tstride + k] = v;
            if (gb_n) gb_n[(size_t)t * C + k] = f2bf(v * scale);
        }
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
    *bytes = place == 1 ? 0 : (((size_t)minibatch * ctc_long_table_bytes(max_time, 64 * ctc_long_vt(max_label_len)) + 255) & ~(size_t)255);
    return OCR_OK;
}
extern "C" int ocr_ctc_loss_long(const float* activations, float* gradients, void* grad_ntc_bf16, float scale, const int* flat_labels,
                                 const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch, int max_time,
                                 int max_label_len, int blank_label, float* costs, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!activations || !flat_labels || !label_lengths || !input_lengths || !costs) return OCR_ERR_INVALID;
    if (alphabet_size <= 0 || minibatch <= 0 || max_time <= 0 || blank_label < 0 || blank_label >= alphabet_size) return OCR_ERR_INVALID;
    size_t need = 0;
    if (ocr_ctc_long_workspace_size(alphabet_size, max_label_len, max_time, minibatch, &need) != OCR_OK) return OCR_ERR_INVALID;
    if (need && (!workspace || workspace_bytes < need)) return OCR_ERR_INVALID;
    return ctc_long_dispatch(activations, gradients, (bf16_t*)grad_ntc_bf16, scale, flat_labels, label_lengths, input_lengths, alphabet_size,
                             minibatch, max_time, max_label_len, blank_label, costs, (float*)workspace, (hipStream_t)stream_, true);
}

// ------------------------------------------------------------------------------------------------------------------
// Wide alphabets (1 <= C <= 16384, 1 <= L <= 255): the class-wide work on the whole chip, the recursion on one workgroup per sample.  The
// kernels above keep acc[CTC_NW][C] in LDS and give a sample's whole softmax to one workgroup; here that work is two launches, ordered by
// the stream (no workgroup waits on another):
//   ctc_wide_rows_kernel     one workgroup per logit row (t, n).  The row is read once into registers (16 elements a thread); the workgroup
//                            reduces max and sum, writes softmax (* scale) to the bf16 [N][T][C] and / or f32 [T][N][C] gradient as if no
//                            label were there, and gathers logy[t][s] = a[lab[s]] - lse into the sample's table in the workspace, in
//                            ctc_long_kernel's [T][SP] layout.  Rows with t >= Tn and all rows of an infeasible sample are zeros.
//   ctc_wide_samples_kernel  one workgroup per sample: ctc_long_recursions on that table (alpha, beta beside it in the workspace), then the
//                            fix-up: per frame the slot posteriors are summed per class through the class's first slot (canon[s]; every blank
//                            slot is slot 0), so a wave's accumulator is [SP] floats, not [C], and each first slot overwrites its one gradient
//                            element with exp(logy) - sum, rounded once from float32.
// Every workgroup of both kernels derives its sample's label offset, extended label and feasibility itself (ctc_wide_sample).
// ------------------------------------------------------------------------------------------------------------------
constexpr int CTC_WIDE_MAX_C = 16384;
constexpr int CTC_WIDE_PER = 16;        // row elements a thread of the rows kernel keeps: 256 threads cover C <= 4096, 512 cover 8192, 1024 cover 16384

// lab[SP] = the sample's extended label (blank beyond S); -> feasible.  cnt = two shared ints; ends with a __syncthreads()
__device__ __forceinline__ bool ctc_wide_sample(const int* __restrict__ flat_labels, const int* __restrict__ label_len, int n, int L, int Tn, int SP,
                                                int blank, int* lab, int* cnt) {
    const int tid = threadIdx.x, nt = blockDim.x, S = 2 * L + 1;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    int part = 0;                          // exclusive prefix sum of the label lengths
    for (int i = tid; i < n; i += nt) part += label_len[i];
    if (part) atomicAdd(&cnt[0], part);
    __syncthreads();
    const int* labels = flat_labels + cnt[0];
    const bool fits = L >= 0 && S <= SP;   // a label longer than the declared capacity has no table: treated like an infeasible sample
    int rep = 0;
    for (int s = tid; s < SP; s += nt) {
        const bool in = fits && s < S;
        lab[s] = (in && (s & 1)) ? labels[s >> 1] : blank;
        if (in && (s & 1) && s >= 3 && labels[s >> 1] == labels[(s >> 1) - 1]) rep++;
    }
    if (rep) atomicAdd(&cnt[1], rep);
    __syncthreads();
    return fits && Tn > 0 && L + cnt[1] <= Tn;
}

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
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int k = (i * NT + tid) * VEC;
        const bool in = t < Tn && k < C;              // (k < C covers k + VEC <= C: C is a multiple of VEC)
        if constexpr (VEC == 1) v[i] = in ? row[k] : NEG_INF;
        else {
#pragma unroll
            for (int q = 0; q < VEC / 4; ++q) {
                const f32x4 x = in ? *(const f32x4*)(row + k + 4 * q) : (f32x4){NEG_INF, NEG_INF, NEG_INF, NEG_INF};
                v[i * VEC + 4 * q] = x.x; v[i * VEC + 4 * q + 1] = x.y; v[i * VEC + 4 * q + 2] = x.z; v[i * VEC + 4 * q + 3] = x.w;
            }
        }
    }
    const bool live = ctc_wide_sample(flat_labels, label_len, n, L, Tn, SP, blank, lab, s_cnt) && t < Tn;

    float inv = 0.f, lse = 0.f;
    if (live) {
        float m = v[0];
#pragma unroll
        for (int j = 1; j < CTC_WIDE_PER; ++j) m = fmaxf(m, v[j]);
        m = wave_max(m);
        if (lane == 0) s_max[wave] = m;
        __syncthreads();
        m = s_max[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, s_max[w]);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < CTC_WIDE_PER; ++j) { v[j] = __expf(v[j] - m); sum += v[j]; }      // (elements past C: exp(-inf) = 0)
        sum = wave_sum(sum);
        if (lane == 0) s_sum[wave] = sum;
        __syncthreads();
        sum = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += s_sum[w];
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

    if (!ctc_wide_sample(flat_labels, label_len, n, L, Tn, SP, blank, lab, s_cnt)) { if (tid == 0) costs[n] = 0.f; return; }
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
            if (s < S) {
                const float al = alpha[base + v * 64], be = beta[base + v * 64];
                if (al != NEG_INF && be != NEG_INF) atomicAdd(&wacc[canon[s]], expf(al + be - ly[v] - logp));
            }
        }
#pragma unroll
        for (int v = 0; v < VT; ++v) {
            const int s = lane * VT + v;
            if (s < S && canon[s] == s) {
                const float g = expf(ly[v]) - wacc[s];
                const int k = lab[s];
                if (g_n) g_n[t * tstride + k] = g;
                if (gb_n) gb_n[(size_t)t * C + k] = f2bf(g * scale);
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
    *bytes = ((size_t)minibatch * ctc_long_table_bytes(max_time, 64 * ctc_long_vt(max_label_len)) + 255) & ~(size_t)255;
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
    if (!activations || !flat_labels || !label_lengths || !input_lengths || !costs || !workspace) return OCR_ERR_INVALID;
    if (blank_label < 0 || blank_label >= alphabet_size || (long)minibatch * max_time > 0x7fffffffL) return OCR_ERR_INVALID;
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
