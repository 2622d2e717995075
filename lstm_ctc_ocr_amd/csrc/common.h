// Shared device/host helpers for the gfx950 (MI355X, CDNA4) CRNN-OCR kernels.
// Everything in this directory is written for wave64 / MFMA / 160 KiB LDS only;
// there is deliberately no other backend.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <atomic>

#define OCR_WAVE 64

// Status codes mirror warp-ctc's ctcStatus_t numbering (0 ok, 1 memops, 2 invalid
// value, 3 execution failed) so a caller written against that ABI keeps working.
enum {
    OCR_OK = 0,
    OCR_ERR_MEMOPS = 1,
    OCR_ERR_INVALID = 2,
    OCR_ERR_EXEC = 3,
};

#define OCR_CHECK_LAUNCH()                                        \
    do {                                                          \
        hipError_t e__ = hipGetLastError();                       \
        if (e__ != hipSuccess) return OCR_ERR_EXEC;               \
    } while (0)

typedef uint16_t bf16_t;  // raw bfloat16 bits in HBM
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// round-to-nearest-even fp32 -> bf16 (same rule as torch's .to(bfloat16)); NaN kept quiet.
__device__ __forceinline__ bf16_t f2bf(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
// two floats -> packed bf16 pair with ONE v_cvt_pk_bf16_f32 (gfx950 native, round-to-nearest-even like f2bf)
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    bf16x2_t v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float bf_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }

// The routing codes of a max-pool window for one 8-channel group, 4 bits per channel, channel c at bits 4c .. 4c + 3: bits 0-1 the index of the
// FIRST maximum in TF scan order (a * kh + b, a over W), bit 2 = (maximum > 0), bit 3 clear — from the window's packed bf16 rows, i.e. compared
// on the values a storing forward pass writes, with the comparisons maxpool_bwd_kernel makes on the stored tensor.  One format for every
// producer (conv1.hip, pool.hip, batchnorm.hip, conv_k3.hip, conv_ws.hip) and consumer of codes.
template <int CNT>
__device__ __forceinline__ uint32_t pool_code_word(const u32x4 (&rows)[CNT]) {
    uint32_t word = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float v[CNT];
#pragma unroll
        for (int e = 0; e < CNT; ++e) {
            const uint32_t pr = c < 2 ? rows[e].x : c < 4 ? rows[e].y : c < 6 ? rows[e].z : rows[e].w;
            v[e] = (c & 1) ? bf_hi(pr) : bf_lo(pr);
        }
        int best = 0; float bv = v[0];
#pragma unroll
        for (int e = 1; e < CNT; ++e) if (v[e] > bv) { bv = v[e]; best = e; }
        word |= (uint32_t)(best | ((bv > 0.f) ? 4 : 0)) << (4 * c);
    }
    return word;
}

// The same codes in packed 16-bit integer arithmetic, two channels per instruction, for windows of post-ReLU values: those are bit patterns
// 0 .. 0x7F80 that order like the floats, so "first maximum" is the first element equal to the integer maximum.  p[e] = element e of the window
// as a packed bf16 pair; ne[e] = min(m - p[e], 1) is 0 where element e is a maximum, and the index of the first such e is
// ne0 * (1 + ne1 * (1 + ne2)) (two elements: ne0).  Returns the two channels' codes at bits 0-2 and 16-18 and leaves the window's packed maximum
// (= the pooled output: rounding is monotone) in mx.
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
template <int CNT>
__device__ __forceinline__ uint32_t pool_code2_u16(const uint32_t (&p)[CNT], uint32_t& mx) {
    const u16x2_t one = {1, 1};
    u16x2_t v[CNT];
#pragma unroll
    for (int e = 0; e < CNT; ++e) v[e] = __builtin_bit_cast(u16x2_t, p[e]);
    u16x2_t m = v[0];
#pragma unroll
    for (int e = 1; e < CNT; ++e) m = __builtin_elementwise_max(m, v[e]);
    u16x2_t t = __builtin_elementwise_min((u16x2_t)(m - v[CNT - 2]), one);
#pragma unroll
    for (int e = CNT - 3; e >= 0; --e) t = __builtin_elementwise_min((u16x2_t)(m - v[e]), one) * (u16x2_t)(t + one);
    const u16x2_t code = t + (u16x2_t)(__builtin_elementwise_min(m, one) << (u16x2_t){2, 2});
    mx = __builtin_bit_cast(uint32_t, m);
    return __builtin_bit_cast(uint32_t, code);
}
// four such pairs -> one word, channel c at bits 4c .. 4c + 2
__device__ __forceinline__ uint32_t pool_code2_merge(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    return ((c0 | (c0 >> 12)) & 0xffu) | (((c1 | (c1 >> 12)) & 0xffu) << 8) | (((c2 | (c2 >> 12)) & 0xffu) << 16) | ((c3 | (c3 >> 12)) << 24);
}

// Helpers of the streaming kernels that more than one of conv1.hip, pool.hip, batchnorm.hip and stream_ops.hip use.
// 16 bytes = four packed bf16 pairs -> eight floats
__device__ __forceinline__ void unpack8(u32x4 p, float* f) {
    f[0] = bf_lo(p.x); f[1] = bf_hi(p.x); f[2] = bf_lo(p.y); f[3] = bf_hi(p.y);
    f[4] = bf_lo(p.z); f[5] = bf_hi(p.z); f[6] = bf_lo(p.w); f[7] = bf_hi(p.w);
}
// element-wise maximum of packed bf16 pairs (2 / 8 values)
__device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b) {
    // bf16 max is exact: keep the raw bits of the larger half (first operand wins ties)
    uint32_t lo = (bf_lo(b) > bf_lo(a)) ? (b & 0xffffu) : (a & 0xffffu);
    uint32_t hi = (bf_hi(b) > bf_hi(a)) ? (b & 0xffff0000u) : (a & 0xffff0000u);
    return lo | hi;
}
__device__ __forceinline__ u32x4 max8(u32x4 a, u32x4 b) {
    u32x4 r = {max2(a.x, b.x), max2(a.y, b.y), max2(a.z, b.z), max2(a.w, b.w)};
    return r;
}
// conv5 dgrad overlap-add, eight channels: unit idx of dx [Nb][W][HC / 8] = col[n][w][0:HC] + col[n][w-1][HC:2HC] (col rows exist for w < W-1),
// the two-term sum (0 + a) + b rounded to bf16 once — conv5_col2im8_kernel's element, and what bn_bwd_stats_col_kernel routes
__device__ __forceinline__ u32x4 col2im_unit8(const bf16_t* __restrict__ col, unsigned idx, int W, int HC) {
    const unsigned hc8 = (unsigned)HC >> 3;
    const unsigned e = (idx % hc8) * 8u, q = idx / hc8;
    const unsigned w = q % (unsigned)W, n = q / (unsigned)W;
    float a[8], b[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { a[c] = 0.f; b[c] = 0.f; }
    const long r0 = ((long)n * (W - 1) + w) * 2L;                    // column row of output position (n, w), first kernel row
    if ((int)w < W - 1) unpack8(*(const u32x4*)(col + r0 * HC + e), a);
    if (w > 0) unpack8(*(const u32x4*)(col + (r0 - 1) * HC + e), b);       // (n, w - 1), second kernel row
    bf16_t o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = f2bf((0.f + a[c]) + b[c]);
    u32x4 pk = {(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16),
                (uint32_t)o[4] | ((uint32_t)o[5] << 16), (uint32_t)o[6] | ((uint32_t)o[7] << 16)};
    return pk;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
#define NEG_INF (-INFINITY)
// whole-wave shifts by one lane as DPP moves (wave_shr:1 / wave_shl:1, one VALU instruction; the lane shifted in takes `fill`)
// instead of ds_bpermute round trips through the LDS crossbar: they sit on the T-sequential critical path of the recursions
__device__ __forceinline__ float wave_shr1(float v, float fill) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float v, float fill) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}
// Block-level reduction over the row lanes of a (row lane) x (channel group) thread layout, followed by one
// atomic (STORE = false) or one plain store (STORE = true: dst is this block's private partial row) per channel.
// red must hold 256*8 floats.
template <typename AccT, bool STORE = false>
__device__ __forceinline__ void block_channel_reduce(const float (&v)[8], float* red, AccT* dst, int C, int groups,
                                                     int rl, int gq, int rlanes) {
    __syncthreads();
    if (rl < rlanes) {
#pragma unroll
        for (int c = 0; c < 8; ++c) red[rl * C + gq * 8 + c] = v[c];
    }
    __syncthreads();
    for (int ch = threadIdx.x; ch < C; ch += 256) {
        float t = 0.f;
        for (int r = 0; r < rlanes; ++r) t += red[r * C + ch];
        if (STORE) dst[ch] = (AccT)t;
        else atomicAdd(&dst[ch], (AccT)t);
    }
}

// hardware-rate gate non-linearities: v_exp_f32 + v_rcp_f32 (relative error ~1e-6, far below the bf16 storage of h)
__device__ __forceinline__ float sigmoidf_(float x) { return __frcp_rn(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) {
    float e = __expf(-2.0f * fabsf(x));          // in (0, 1]: no overflow
    float t = (1.0f - e) * __frcp_rn(1.0f + e);
    return copysignf(t, x);
}

int ocr_cu_count();        // CUs of the current device, 256 while none is visible (gemm.hip; host-only plan queries)

// Tuning knobs (tile policies, stage counts, ...): read from the environment only by `make EXPERIMENTS=1` builds — the A/B tools load that
// library through OCR_NATIVE_LIB; the product library uses the measured defaults.  Kernel-selection knobs that the parity tests force
// are read by both: OCR_CONV_K2 / OCR_CONV_K3 / OCR_K2_CFG / OCR_CONV_WS / OCR_LSTM_PROTO / OCR_LSTM_ROWS (tests/test_gpu_kernels.py) and
// OCR_W9_PLANES / OCR_W9P_GENW / OCR_TN3_NST, with the engine generations OCR_GEMM_ENGINE / OCR_WGRAD_ENGINE
// (tests/test_gpu_kernel_generations.py); DESIGN section 8 has the table.  The 3x3 convolution's knobs, of both kinds, are all read in one
// place: gemm.hip's read_conv_knobs().
static inline const char* ocr_tune_env(const char* name) {
#ifdef OCR_EXPERIMENTS
    return getenv(name);
#else
    (void)name; return nullptr;
#endif
}
// Clock diagnostic of the convolution kernels (ocr_conv_halo_clock_debug, device int64[8]): workgroup 0's first thread stamps
// {shader-clock counter (s_memtime), 100 MHz wall clock (s_memrealtime)} into [0], [1] at entry and [2], [3] at exit, and ADDS its lifetime to
// [4] (shader clocks), [5] (wall ticks), [6] (launches): launches of one stream are serial, so plain adds do.  MHz = [4] / [5] * 100 over
// every stamped launch of a run — the counter passes divide the matrix pipes' busy cycles by the kernels' OWN cycles with it.
__device__ __forceinline__ long long ocr_wall_clock() { return (long long)__builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ void ocr_clk_enter(long long* clk) {
    clk[0] = (long long)__builtin_amdgcn_s_memtime(); clk[1] = ocr_wall_clock();
}
__device__ __forceinline__ void ocr_clk_exit(long long* clk) {
    const long long c = (long long)__builtin_amdgcn_s_memtime(), t = ocr_wall_clock();
    clk[2] = c; clk[3] = t;
    clk[4] += c - clk[0]; clk[5] += t - clk[1]; clk[6] += 1;
}
__host__ __device__ static inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
// blocks of 256 threads for `total` work items of a grid-stride kernel: at least one, at most `cap`
static inline int grid_for(long total, int cap = 4096) {
    long b = (total + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// Lets KERNEL launch with `bytes` of dynamic LDS on the current device (hipFuncSetAttribute MaxDynamicSharedMemorySize): called before
// every launch, it sets the attribute the first time a device needs that much for this kernel instance and is a load otherwise.
#define OCR_MAX_DEVICES 64
template <auto KERNEL>
static inline hipError_t ocr_allow_lds(int bytes) {
    static std::atomic<int> allowed[OCR_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= OCR_MAX_DEVICES) return hipErrorInvalidDevice;
    int have = allowed[dev].load(std::memory_order_acquire);
    if (bytes <= have) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    while (have < bytes && !allowed[dev].compare_exchange_weak(have, bytes, std::memory_order_acq_rel)) {}
    return hipSuccess;
}
