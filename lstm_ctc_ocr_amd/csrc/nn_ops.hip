// HBM-bound layers of the reference graph for gfx950 (SURVEY.md §8a rows a2 conv1, a3, a4):
// conv1 (C_in = 1, K = 9: VALU, not MFMA), max-pool fwd/bwd, training-mode batch-norm fwd/bwd,
// bias-gradient column sums, weight (re)packing.  Everything moves 16 B per lane (8 bf16 / 4 f32),
// coalesced along the channel axis of the reference layout [N, W, H, C].
#include "common.h"
#include <stdlib.h>
#include <algorithm>

__device__ __forceinline__ void unpack8(u32x4 p, float* f) {
    f[0] = bf_lo(p.x); f[1] = bf_hi(p.x); f[2] = bf_lo(p.y); f[3] = bf_hi(p.y);
    f[4] = bf_lo(p.z); f[5] = bf_hi(p.z); f[6] = bf_lo(p.w); f[7] = bf_hi(p.w);
}

// ============================================================================================
// conv1: x f32 [Nb, W, H] (single channel) -> y bf16 [Nb, W, H, Cout], 3x3 SAME, + bias, ReLU
//   reference: conv_single(3,3,64,1,1,'conv1',c_i=1)  lib/networks/LSTM_train.py:24, network.py:160-191
// ============================================================================================
__global__ __launch_bounds__(256) void conv1_fwd_kernel(const float* __restrict__ x,
                                                        const float* __restrict__ w,   // [9][Cout]
                                                        const float* __restrict__ bias,
                                                        bf16_t* __restrict__ y, int Nb, int W, int H,
                                                        int Cout, int relu) {
    // thread = (channel group of 8, pixel lane); its 72 weights + 8 biases stay in registers for the whole grid-stride
    // loop (the first version re-read them from LDS per pixel: 80 ds_reads per 16-B store, 1.3 TB/s)
    const int groups = Cout >> 3;                 // 8 at Cout = 64
    const int gq = threadIdx.x % groups;
    const int plane = threadIdx.x / groups;
    const int planes = 256 / groups;
    float wr[9][8], br[8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) wr[t][c] = w[t * Cout + gq * 8 + c];
#pragma unroll
    for (int c = 0; c < 8; ++c) br[c] = bias[gq * 8 + c];
    const long npix = (long)Nb * W * H;
    for (long pix = (long)blockIdx.x * planes + plane; pix < npix; pix += (long)gridDim.x * planes) {
        int h = (int)(pix % H);
        long q = pix / H;
        int wq = (int)(q % W);
        const float* xn = x + (q - wq) * H;   // start of sample's [W][H] plane
        float xv[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            int ww = wq + t / 3 - 1, hh = h + t % 3 - 1;
            xv[t] = ((unsigned)ww < (unsigned)W && (unsigned)hh < (unsigned)H) ? xn[(long)ww * H + hh] : 0.f;
        }
        float o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] = fmaf(xv[t], wr[t][c], o[c]);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            o[c] += br[c];
            if (relu) o[c] = fmaxf(o[c], 0.f);
        }
        u32x4 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
        *(u32x4*)(y + pix * Cout + gq * 8) = pk;
    }
}

// conv1 weight/bias gradient: dW[9][Cout] += sum_pix x[shifted] * dz[pix][:],  db[Cout] += sum_pix dz
// Each block owns a contiguous pixel chunk; thread = (channel group of 8) x (pixel lane of 32).
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const float* __restrict__ x,
                                                          const bf16_t* __restrict__ dz,
                                                          float* __restrict__ dw, float* __restrict__ db,
                                                          int Nb, int W, int H, int Cout, int pix_per_block) {
    // requires Cout == 64: 8 channel groups x 32 pixel lanes = 256 threads
    const int gq = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const long npix = (long)Nb * W * H;
    const long p0 = (long)blockIdx.x * pix_per_block;
    const long p1 = min(npix, p0 + pix_per_block);
    float acc[10][8];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[t][c] = 0.f;
    for (long pix = p0 + pl; pix < p1; pix += 32) {
        int h = (int)(pix % H);
        long q = pix / H;
        int wq = (int)(q % W);
        const float* xn = x + (q - wq) * H;
        u32x4 d = *(const u32x4*)(dz + pix * Cout + gq * 8);
        float dv[8] = {bf_lo(d.x), bf_hi(d.x), bf_lo(d.y), bf_hi(d.y), bf_lo(d.z), bf_hi(d.z), bf_lo(d.w), bf_hi(d.w)};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            int ww = wq + t / 3 - 1, hh = h + t % 3 - 1;
            float xv = ((unsigned)ww < (unsigned)W && (unsigned)hh < (unsigned)H) ? xn[(long)ww * H + hh] : 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[t][c] = fmaf(xv, dv[c], acc[t][c]);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[9][c] += dv[c];
    }
    // reduce the 32 pixel lanes: lanes of one wave hold pl = 8 consecutive values -> shuffle over pl bits,
    // then 4 waves through LDS
    __shared__ float red[4][10][64];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v = acc[t][c];
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            acc[t][c] = v;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 8) {
#pragma unroll
        for (int t = 0; t < 10; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) red[wave][t][lane * 8 + c] = acc[t][c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 10 * 64; i += 256) {
        int t = i / 64, c = i % 64;
        float v = red[0][t][c] + red[1][t][c] + red[2][t][c] + red[3][t][c];
        if (t < 9) atomicAdd(dw + t * Cout + c, v);
        else atomicAdd(db + c, v);
    }
}

// ============================================================================================
// conv1 + ReLU + 2x2 max-pool fused (forward) and its fused backward (pool routing + ReLU mask + conv1 weight gradient).
// conv1's full-resolution output (N*W*H*64 bf16 = 67 MB at batch 64) is the largest tensor of the network and is only
// ever consumed by pool1; with K = 9 it is cheaper to recompute than to store: the forward writes only the pooled map,
// the backward recomputes the 2x2 window (identical fp32 arithmetic, hence identical arg-max and ReLU mask), routes the
// pooled gradient to the first maximum (TF scan order: W outer, H inner) and accumulates dW / db in registers.
//   reference: LSTM_train.py:24-25 (conv_single 3x3 c_i=1 -> max_pool 2,2), network.py:160-191, 343-350
// ============================================================================================
// the 2x2 window's 4 x 8 outputs from its 4 x 4 patch: nine fused multiply-adds in tap order, + bias, ReLU
__device__ __forceinline__ void conv1_window_fma(const float (&patch)[4][4], const float (&wr)[9][8], const float (&br)[8], float (&o)[4][8]) {
    // channel PAIRS per instruction (v_pk_fma_f32: two fp32 FMAs per lane at the rate of one — the kernel is VALU-bound): the same fused
    // multiply-adds in the same order per channel, hence bit-identical results (round 4)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int a = e >> 1, b = e & 1;               // window element (a over W, b over H) = TF scan order
        f32x2 acc2[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc2[q] = (f32x2){0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float pv = patch[a + t / 3][b + t % 3];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc2[q] = __builtin_elementwise_fma((f32x2){pv, pv}, (f32x2){wr[t][2 * q], wr[t][2 * q + 1]}, acc2[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o[e][2 * q] = fmaxf(acc2[q].x + br[2 * q], 0.f);
            o[e][2 * q + 1] = fmaxf(acc2[q].y + br[2 * q + 1], 0.f);
        }
    }
}

#ifdef OCR_EXPERIMENTS   // the first generation (OCR_CONV1_GEN=1): every lane loads its own patch from HBM; kept to measure the tile kernels below against
// 4x4 input patch around the 2x2 output window (rows w0-1..w0+2, cols h0-1..h0+2), zero outside the image
__device__ __forceinline__ void conv1_patch(const float* __restrict__ xn, int W, int H, int w0, int h0, float (&patch)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ww = w0 - 1 + i, hh = h0 - 1 + j;
            patch[i][j] = ((unsigned)ww < (unsigned)W && (unsigned)hh < (unsigned)H) ? xn[(long)ww * H + hh] : 0.f;
        }
}
// arg-max of the 2x2 window on the bf16-ROUNDED outputs (what the forward stores and an unfused max-pool backward would compare: ties resolve
// to the first element in TF scan order) and the ReLU bit of the winner: code = best | (winner > 0) << 2
__device__ __forceinline__ int conv1_pool_code(float o0, float o1, float o2, float o3) {
    const float r[4] = {bf_lo(pack_bf2(o0, 0.f)), bf_lo(pack_bf2(o1, 0.f)), bf_lo(pack_bf2(o2, 0.f)), bf_lo(pack_bf2(o3, 0.f))};
    int best = 0; float bvv = r[0];
#pragma unroll
    for (int e = 1; e < 4; ++e) if (r[e] > bvv) { bvv = r[e]; best = e; }
    return best | ((bvv > 0.f) ? 4 : 0);
}
__device__ __forceinline__ void conv1_window(const float* __restrict__ xn, int W, int H, int w0, int h0,
                                             const float (&wr)[9][8], const float (&br)[8], float (&o)[4][8], float (&patch)[4][4]) {
    conv1_patch(xn, W, H, w0, h0, patch);
    conv1_window_fma(patch, wr, br, o);
}
#endif

#ifdef OCR_EXPERIMENTS   // measured and rejected: compiled, reachable (OCR_CONV1_V2=1) and tested only in the experiments flavour
// Second generation of the two fused kernels (round 2; behind OCR_CONV1_V2=1 — measured slightly SLOWER than the first, see conv1_v1()).  The ISA of the first showed, per
// loop iteration, two 64-bit integer divisions (~130 instructions each, half of them scalar with readfirstlane round trips), 16 patch
// loads each in its own exec-masked branch, and the loads placed right in front of their first use — so every iteration exposed a
// whole memory round trip.  Here: 32-bit index arithmetic, branch-free patch loads (clamped address, then a select: rows 1-2 and
// columns 1-2 of the 4 x 4 patch are always inside the image), and the NEXT iteration's patch (and gradient row) requested before
// the current iteration's ~300 FMAs.  The arithmetic on the loaded values is unchanged, hence bit-identical results.
struct Conv1Patch { float v[4][4]; };
struct Conv1Raw { float t[4][4]; unsigned ok; };     // as loaded (clamped addresses) + which border rows / columns exist; selected later
__device__ __forceinline__ void conv1_patch_load(const float* __restrict__ x, int W, int H, int Wo, int Ho, unsigned op, Conv1Raw& raw) {
    const unsigned ho = op % (unsigned)Ho, q = op / (unsigned)Ho;
    const unsigned wo = q % (unsigned)Wo, n = q / (unsigned)Wo;
    const float* xn = x + (long)n * W * H;
    const int w0 = (int)wo * 2, h0 = (int)ho * 2;
    // rows w0 - 1 .. w0 + 2: only the first can be < 0, only the last can be >= W (likewise the columns)
    const bool r0 = w0 > 0, r3 = w0 + 2 < W, c0 = h0 > 0, c3 = h0 + 2 < H;
    const int wi[4] = {r0 ? w0 - 1 : 0, w0, w0 + 1, r3 ? w0 + 2 : w0 + 1};
    const int hj[4] = {c0 ? h0 - 1 : 0, h0, h0 + 1, c3 ? h0 + 2 : h0 + 1};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) raw.t[i][j] = xn[wi[i] * H + hj[j]];
    raw.ok = (r0 ? 1u : 0u) | (r3 ? 2u : 0u) | (c0 ? 4u : 0u) | (c3 ? 8u : 0u);
}
// the zero padding is applied when the patch is USED (one iteration after its loads were issued): a select right behind the loads
// would make the wave wait for them before the current iteration's arithmetic
__device__ __forceinline__ void conv1_patch_select(const Conv1Raw& raw, Conv1Patch& pt) {
    const bool r0 = raw.ok & 1u, r3 = raw.ok & 2u, c0 = raw.ok & 4u, c3 = raw.ok & 8u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = (i != 0 || r0) && (i != 3 || r3) && (j != 0 || c0) && (j != 3 || c3);
            pt.v[i][j] = ok ? raw.t[i][j] : 0.f;
        }
}
// The 80 weight / bias registers are made "arrived" before the loop: the memory counter is in-order, so as long as the compiler has to
// assume that a weight load may still be outstanding, its counted waits inside the loop also drain the NEXT iteration's prefetch.
__device__ __forceinline__ void conv1_pin_weights(float (&wr)[9][8], float (&br)[8]) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) asm volatile("" : "+v"(wr[t][c]));
#pragma unroll
    for (int c = 0; c < 8; ++c) asm volatile("" : "+v"(br[c]));
}
__device__ __forceinline__ void conv1_window_compute(const Conv1Patch& pt, const float (&wr)[9][8], const float (&br)[8], float (&o)[4][8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int a = e >> 1, b = e & 1;               // window element (a over W, b over H) = TF scan order
#pragma unroll
        for (int c = 0; c < 8; ++c) o[e][c] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) o[e][c] = fmaf(pt.v[a + t / 3][b + t % 3], wr[t][c], o[e][c]);
#pragma unroll
        for (int c = 0; c < 8; ++c) o[e][c] = fmaxf(o[e][c] + br[c], 0.f);
    }
}

__global__ __launch_bounds__(256) void conv1_pool_fwd2_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, bf16_t* __restrict__ p,
                                                              int Nb, int W, int H, int Cout) {
    const int groups = Cout >> 3, gq = threadIdx.x % groups, plane = threadIdx.x / groups, planes = 256 / groups;
    float wr[9][8], br[8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) wr[t][c] = w[t * Cout + gq * 8 + c];
#pragma unroll
    for (int c = 0; c < 8; ++c) br[c] = bias[gq * 8 + c];
    conv1_pin_weights(wr, br);
    const int Wo = W >> 1, Ho = H >> 1;
    const unsigned npix = (unsigned)Nb * Wo * Ho, stride = gridDim.x * planes;      // npix < 2^31 (checked by the host)
    unsigned op = blockIdx.x * planes + plane;
    Conv1Raw nxt;
    if (op < npix) conv1_patch_load(x, W, H, Wo, Ho, op, nxt);
    for (; op < npix; op += stride) {
        Conv1Patch cur;
        conv1_patch_select(nxt, cur);
        if (op + stride < npix) conv1_patch_load(x, W, H, Wo, Ho, op + stride, nxt);     // in flight during the FMAs below
        float o[4][8];
        conv1_window_compute(cur, wr, br, o);
        float m[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) m[c] = fmaxf(fmaxf(o[0][c], o[1][c]), fmaxf(o[2][c], o[3][c]));   // rounding is monotone: max then round
        u32x4 pk = {pack_bf2(m[0], m[1]), pack_bf2(m[2], m[3]), pack_bf2(m[4], m[5]), pack_bf2(m[6], m[7])};
        *(u32x4*)(p + (long)op * Cout + gq * 8) = pk;
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv1_pool_bwd2_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                            const bf16_t* __restrict__ dp, float* __restrict__ dw, float* __restrict__ db, int Nb, int W,
                            int H, int Cout, int pix_per_block) {
    // Cout == 64: 8 channel groups x 32 pixel lanes
    const int gq = threadIdx.x & 7, pl = threadIdx.x >> 3;
    float wr[9][8], br[8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) wr[t][c] = w[t * Cout + gq * 8 + c];
#pragma unroll
    for (int c = 0; c < 8; ++c) br[c] = bias[gq * 8 + c];
    conv1_pin_weights(wr, br);
    const int Wo = W >> 1, Ho = H >> 1;
    const unsigned npix = (unsigned)Nb * Wo * Ho;
    const unsigned p0 = blockIdx.x * (unsigned)pix_per_block, p1 = min(npix, p0 + (unsigned)pix_per_block);
    float acc[10][8];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[t][c] = 0.f;
    unsigned op = p0 + pl;
    Conv1Raw nxt;
    u32x4 gnxt = {0u, 0u, 0u, 0u};
    if (op < p1) {
        conv1_patch_load(x, W, H, Wo, Ho, op, nxt);
        gnxt = *(const u32x4*)(dp + (long)op * Cout + gq * 8);
    }
    for (; op < p1; op += 32) {
        Conv1Patch cur;
        conv1_patch_select(nxt, cur);
        const u32x4 gcur = gnxt;
        if (op + 32 < p1) {                                 // the next iteration's operands, in flight during this one's arithmetic
            conv1_patch_load(x, W, H, Wo, Ho, op + 32, nxt);
            gnxt = *(const u32x4*)(dp + (long)(op + 32) * Cout + gq * 8);
        }
        float o[4][8];
        conv1_window_compute(cur, wr, br, o);
        float g[8];
        unpack8(gcur, g);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            // the forward stored bf16(max); compare on the same rounded values so ties resolve exactly like the unfused path
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = bf_lo(pack_bf2(o[e][c], 0.f));
            int best = 0; float bvv = r[0];
#pragma unroll
            for (int e = 1; e < 4; ++e) if (r[e] > bvv) { bvv = r[e]; best = e; }
            const float gv = (bvv > 0.f) ? g[c] : 0.f;             // ReLU mask of the winning element
            acc[9][c] += gv;
            const int a = best >> 1, b = best & 1;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int i = t / 3, j = t % 3;
                const float xv = (a == 0) ? ((b == 0) ? cur.v[i][j] : cur.v[i][j + 1]) : ((b == 0) ? cur.v[i + 1][j] : cur.v[i + 1][j + 1]);
                acc[t][c] = fmaf(xv, gv, acc[t][c]);
            }
        }
    }
    __shared__ float red[4][10][64];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v = acc[t][c];
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            acc[t][c] = v;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 8) {
#pragma unroll
        for (int t = 0; t < 10; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) red[wave][t][lane * 8 + c] = acc[t][c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 10 * 64; i += 256) {
        int t = i / 64, c = i % 64;
        float v = red[0][t][c] + red[1][t][c] + red[2][t][c] + red[3][t][c];
        if (t < 9) atomicAdd(dw + t * Cout + c, v);
        else atomicAdd(db + c, v);
    }
}
#endif   // OCR_EXPERIMENTS (second-generation conv1 + pool kernels)

#ifdef OCR_EXPERIMENTS   // first generation, continued: the grid-stride forward and the private-patch backward
template <bool CODES>
__device__ __forceinline__ void conv1_pool_fwd_body(const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ bias, bf16_t* __restrict__ p,
                                                    int Nb, int W, int H, int Cout, f32x4* __restrict__ zero, long zero_n4,
                                                    uint32_t* __restrict__ codes, u32x4* __restrict__ ones, long ones_n4) {
    // the step's flat gradient buffer is cleared by the FIRST kernel of the forward pass (round 4: it was a fill launch of its own): the
    // stores go out here and drain beside the VALU-bound work below.  Likewise `ones`: the hand-off blocks of the step's persistent LSTM
    // launches, set to the all-ones pattern they start from (ocr_lstm_*_seq2 with OCR_LSTM_PREPARED: two fill launches less).
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < zero_n4; i += (long)gridDim.x * 256) zero[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < ones_n4; i += (long)gridDim.x * 256) ones[i] = (u32x4){~0u, ~0u, ~0u, ~0u};
    const int groups = Cout >> 3, gq = threadIdx.x % groups, plane = threadIdx.x / groups, planes = 256 / groups;
    float wr[9][8], br[8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) wr[t][c] = w[t * Cout + gq * 8 + c];
#pragma unroll
    for (int c = 0; c < 8; ++c) br[c] = bias[gq * 8 + c];
    const int Wo = W >> 1, Ho = H >> 1;
    const long npix = (long)Nb * Wo * Ho;
    for (long op = (long)blockIdx.x * planes + plane; op < npix; op += (long)gridDim.x * planes) {
        const int ho = (int)(op % Ho);
        const long q = op / Ho;
        const int wo = (int)(q % Wo);
        const long n = q / Wo;
        float o[4][8], patch[4][4];
        conv1_window(x + n * W * H, W, H, wo * 2, ho * 2, wr, br, o, patch);
        float m[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) m[c] = fmaxf(fmaxf(o[0][c], o[1][c]), fmaxf(o[2][c], o[3][c]));   // rounding is monotone: max then round
        u32x4 pk = {pack_bf2(m[0], m[1]), pack_bf2(m[2], m[3]), pack_bf2(m[4], m[5]), pack_bf2(m[6], m[7])};
        *(u32x4*)(p + op * Cout + gq * 8) = pk;
        if constexpr (CODES) {        // training: the pool's routing and the ReLU bit per output, 4 bits each — the backward pass need not recompute the window
            uint32_t word = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) word |= (uint32_t)conv1_pool_code(o[0][c], o[1][c], o[2][c], o[3][c]) << (4 * c);
            codes[op * groups + gq] = word;
        }
    }
}

template <bool CODES>
__global__ __launch_bounds__(256) void conv1_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             bf16_t* __restrict__ p, int Nb, int W, int H, int Cout, f32x4* __restrict__ zero,
                                                             long zero_n4, uint32_t* __restrict__ codes, u32x4* __restrict__ ones, long ones_n4) {
    conv1_pool_fwd_body<CODES>(x, w, bias, p, Nb, W, H, Cout, zero, zero_n4, codes, ones, ones_n4);
}
template <bool CODES /* routing + ReLU bits from the forward pass: no window recomputation, and none of its 110 registers (weights, outputs) */>
__global__ __launch_bounds__(256) void conv1_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const bf16_t* __restrict__ dp,
                                                             float* __restrict__ dw, float* __restrict__ db, int Nb, int W,
                                                             int H, int Cout, int pix_per_block, const uint32_t* __restrict__ codes,
                                                             float* __restrict__ slab) {
    // Cout == 64: 8 channel groups x 32 pixel lanes
    const int gq = threadIdx.x & 7, pl = threadIdx.x >> 3;
    float wr[CODES ? 1 : 9][8], br[8];
    if (!CODES) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) wr[CODES ? 0 : t][c] = w[t * Cout + gq * 8 + c];
#pragma unroll
        for (int c = 0; c < 8; ++c) br[c] = bias[gq * 8 + c];
    }
    const int Wo = W >> 1, Ho = H >> 1;
    const long npix = (long)Nb * Wo * Ho;
    const long p0 = (long)blockIdx.x * pix_per_block, p1 = min(npix, p0 + pix_per_block);
    float acc[10][8];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[t][c] = 0.f;
    __shared__ float patch_lds[256 * 17];               // a thread's 4 x 4 patch, stride 17 words: equal indices of a wave's lanes fall into distinct banks
    float* const mypatch = patch_lds + threadIdx.x * 17;
    for (long op = p0 + pl; op < p1; op += 32) {
        const int ho = (int)(op % Ho);
        const long q = op / Ho;
        const int wo = (int)(q % Wo);
        const long n = q / Wo;
        float o[CODES ? 1 : 4][8], patch[4][4];
        uint32_t word = 0;
        if constexpr (CODES) {          // round 4: routing + ReLU bits saved by the forward pass (conv1_pool_code): no recomputation of the window
            conv1_patch(x + n * W * H, W, H, wo * 2, ho * 2, patch);
            word = codes[op * 8 + gq];
        } else {
            conv1_window(x + n * W * H, W, H, wo * 2, ho * 2, wr, br, o, patch);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) mypatch[i * 4 + j] = patch[i][j];
        float g[8];
        unpack8(*(const u32x4*)(dp + op * Cout + gq * 8), g);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            // the forward stored bf16(max); compare on the same rounded values so ties resolve exactly like the unfused path
            int code;
            if constexpr (CODES) code = (int)((word >> (4 * c)) & 7u);
            else code = conv1_pool_code(o[0][c], o[1][c], o[2][c], o[3][c]);
            const int best = code & 3;
            const float gv = (code & 4) ? g[c] : 0.f;              // ReLU mask of the winning element
            acc[9][c] += gv;
            // patch[a + t/3][b + t%3] with a run-time (a, b) PER CHANNEL: looked up in this thread's private LDS copy of the patch (one
            // ds_read with an immediate offset per tap) — as three v_cndmask per tap and channel this was 216 of the ~380 VALU instructions
            // of an iteration (round 4)
            const float* px = mypatch + (best >> 1) * 4 + (best & 1);
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[t][c] = fmaf(px[(t / 3) * 4 + t % 3], gv, acc[t][c]);
        }
    }
    __shared__ float red[4][10][64];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v = acc[t][c];
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            acc[t][c] = v;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 8) {
#pragma unroll
        for (int t = 0; t < 10; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) red[wave][t][lane * 8 + c] = acc[t][c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 10 * 64; i += 256) {
        int t = i / 64, c = i % 64;
        float v = red[0][t][c] + red[1][t][c] + red[2][t][c] + red[3][t][c];
        // slab form (round 4): this block's 640 partial sums go to its own row, the merged slab reduction that follows anyway adds the rows
        // in a fixed order — 512 blocks x 640 same-address atomics were ~10 us of the kernel's 33 (it got SLOWER with more, smaller blocks:
        // profiles/r04k), and the conv1 gradient was the last one that was not bit-reproducible
        if (slab != nullptr) slab[(long)blockIdx.x * 640 + i] = v;
        else if (t < 9) atomicAdd(dw + t * Cout + c, v);
        else atomicAdd(db + c, v);
    }
}
#endif   // OCR_EXPERIMENTS (first-generation conv1 + pool kernels)

// --------------------------------------------------------------------------------------------
// The shipped generation: a block owns a run of consecutive pooled pixels [p0, p1) and stages the input rows they touch in LDS once.
// In memory x is rows of H floats, image n's row w at global row R = n * W + w; pooled column q = n * Wo + wo covers global rows 2q, 2q + 1.  A
// run spans columns q0 .. q1, i.e. rows 2 q0 - 1 .. 2 q1 + 2, which are CONTIGUOUS in x (images follow each other): one coalesced pass loads
// them, zero where the row lies before the first or behind the last image.  Tile row r = global row 2 q0 - 1 + r, stride RS = H + 2 words: word 0
// and word H + 1 of a row are the zero padding left and right of the image.  Pixel (column q0 + qi, ho) takes patch[i][j] from
// tile[(2 qi + i) * RS + 2 ho + j]: no bounds checks.  What a tile cannot express is the halo row of a column at an image's edge — it holds the
// neighbouring image's row, real data for that image's own columns: the first patch row reads as zero where wo == 0, the last where wo == Wo - 1.
// Banks: the lanes of one pixel (its channel groups) read one address (broadcast), neighbouring pixels are 2 words apart, a wave covers 8
// pixels = 16 consecutive words (or, where the run wraps into the next column, words 2 RS = 2 H + 4 further on: distinct banks for H % 16 == 0).
// Divisions: p0 / Ho and q0 % Wo once per block in 32 bits; per pixel v / d = umulhi(v, ceil(2^32 / d)), exact for v * d < 2^32 (the host checks;
// reciprocal 0 stands for d == 1).
struct Conv1Geo { int RS, Ho, Wo; unsigned ho0, wo0, rHo, rWo; };
__device__ __forceinline__ unsigned conv1_div(unsigned v, unsigned r) { return r ? __umulhi(v, r) : v; }
__device__ __forceinline__ Conv1Geo conv1_tile_stage(const float* __restrict__ x, int Nb, int W, int H, unsigned p0, unsigned p1, unsigned rH,
                                                     unsigned rHo, unsigned rWo, float* __restrict__ tile) {
    Conv1Geo g;
    g.RS = H + 2; g.Ho = H >> 1; g.Wo = W >> 1; g.rHo = rHo; g.rWo = rWo;
    const unsigned q0 = p0 / (unsigned)g.Ho, q1 = (p1 - 1) / (unsigned)g.Ho;
    g.ho0 = p0 - q0 * (unsigned)g.Ho; g.wo0 = q0 % (unsigned)g.Wo;
    const int rows = 2 * (int)(q1 - q0 + 1) + 2;
    const long first = (2 * (long)q0 - 1) * H, total = (long)Nb * W * H;       // the tile's first word in x (row -1: before the first image)
    for (unsigned i = threadIdx.x; i < (unsigned)(rows * H); i += 256) {
        const unsigned r = __umulhi(i, rH), h = i - r * (unsigned)H;
        const long e = first + i;
        tile[r * g.RS + 1 + h] = (e >= 0 && e < total) ? x[e] : 0.f;
    }
    for (int r = threadIdx.x; r < rows; r += 256) { tile[r * g.RS] = 0.f; tile[r * g.RS + H + 1] = 0.f; }
    __syncthreads();
    return g;
}
// the run's i-th pixel: where its patch starts in the tile, and whether its first / last patch row lies outside its image
struct Conv1Pix { const float* base; bool top, bottom; };
__device__ __forceinline__ Conv1Pix conv1_tile_pixel(const float* __restrict__ tile, const Conv1Geo& g, unsigned i) {
    const unsigned v = g.ho0 + i, qi = conv1_div(v, g.rHo), ho = v - qi * (unsigned)g.Ho;
    const unsigned c = g.wo0 + qi, wo = c - conv1_div(c, g.rWo) * (unsigned)g.Wo;
    Conv1Pix px = {tile + (2 * qi) * g.RS + 2 * ho, wo == 0, wo == (unsigned)g.Wo - 1};
    return px;
}
__device__ __forceinline__ void conv1_tile_patch(const Conv1Pix& px, int RS, float (&patch)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) patch[a][b] = px.base[a * RS + b];
#pragma unroll
    for (int b = 0; b < 4; ++b) { patch[0][b] = px.top ? 0.f : patch[0][b]; patch[3][b] = px.bottom ? 0.f : patch[3][b]; }
}
// the window's outputs -> its pooled bf16 values (as 4 packed pairs) and routing codes.  Post-ReLU values are >= +0 (an accumulator that starts
// at +0 never becomes -0, so neither does accumulator + bias), hence pool_code2_u16's integer order is the float order: the same first maximum on
// the rounded values, the same ReLU bit, and max-then-round == round-then-max, as conv1_pool_code / the first generation's float max give.
__device__ __forceinline__ uint32_t conv1_pool_pack(const float (&o)[4][8], u32x4& pk) {
    uint32_t m[4], cd[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t pe[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            pe[e] = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){o[e][2 * q], o[e][2 * q + 1]}, bf16x2_t));
        }
        cd[q] = pool_code2_u16(pe, m[q]);
    }
    pk = (u32x4){m[0], m[1], m[2], m[3]};
    return pool_code2_merge(cd[0], cd[1], cd[2], cd[3]);
}

template <bool CODES>
__global__ __launch_bounds__(256) void conv1_pool_fwd_tile_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                  bf16_t* __restrict__ p, int Nb, int W, int H, int Cout, int pix_per_block, unsigned rH,
                                                                  unsigned rHo, unsigned rWo, f32x4* __restrict__ zero, long zero_n4,
                                                                  uint32_t* __restrict__ codes, u32x4* __restrict__ ones, long ones_n4) {
    extern __shared__ float conv1_tile[];
    // the step's flat gradient buffer is cleared by the FIRST kernel of the forward pass (round 4: it was a fill launch of its own): the
    // stores go out here and drain beside the VALU-bound work below.  Likewise `ones`: the hand-off blocks of the step's persistent LSTM
    // launches, set to the all-ones pattern they start from (ocr_lstm_*_seq2 with OCR_LSTM_PREPARED: two fill launches less).
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < zero_n4; i += (long)gridDim.x * 256) zero[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < ones_n4; i += (long)gridDim.x * 256) ones[i] = (u32x4){~0u, ~0u, ~0u, ~0u};
    const unsigned npix = (unsigned)Nb * (W >> 1) * (H >> 1);                       // < 2^31 (checked by the host)
    const unsigned p0 = blockIdx.x * (unsigned)pix_per_block, p1 = min(npix, p0 + (unsigned)pix_per_block);
    if (p0 >= npix) return;                                                         // (an empty batch still gets its fills)
    const int groups = Cout >> 3, gq = threadIdx.x % groups, plane = threadIdx.x / groups, planes = 256 / groups;
    float wr[9][8], br[8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) wr[t][c] = w[t * Cout + gq * 8 + c];
#pragma unroll
    for (int c = 0; c < 8; ++c) br[c] = bias[gq * 8 + c];
    const Conv1Geo geo = conv1_tile_stage(x, Nb, W, H, p0, p1, rH, rHo, rWo, conv1_tile);
    for (unsigned i = plane; i < p1 - p0; i += planes) {
        float o[4][8], patch[4][4];
        conv1_tile_patch(conv1_tile_pixel(conv1_tile, geo, i), geo.RS, patch);
        conv1_window_fma(patch, wr, br, o);
        u32x4 pk;
        const uint32_t word = conv1_pool_pack(o, pk);
        const long op = (long)p0 + i;
        *(u32x4*)(p + op * Cout + gq * 8) = pk;
        // training: the pool's routing and the ReLU bit per output, 4 bits each — the backward pass need not recompute the window
        if constexpr (CODES) codes[op * groups + gq] = word;
    }
}

// The reduction every conv1 + pool backward ends with: lane bits 8, 16, 32 by shuffles, the four waves through LDS, then the block's 640 sums
// to its slab row or, without a slab, to dw / db by atomics.
__device__ __forceinline__ void conv1_bwd_reduce(float (&acc)[10][8], float* __restrict__ dw, float* __restrict__ db, float* __restrict__ slab) {
    __shared__ float red[4][10][64];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v = acc[t][c];
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            acc[t][c] = v;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 8) {
#pragma unroll
        for (int t = 0; t < 10; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) red[wave][t][lane * 8 + c] = acc[t][c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 10 * 64; i += 256) {
        int t = i / 64, c = i % 64;
        float v = red[0][t][c] + red[1][t][c] + red[2][t][c] + red[3][t][c];
        // slab form (round 4): this block's 640 partial sums go to its own row, the merged slab reduction that follows anyway adds the rows
        // in a fixed order — 512 blocks x 640 same-address atomics were ~10 us of the kernel's 33 (it got SLOWER with more, smaller blocks:
        // profiles/r04k), and the conv1 gradient was the last one that was not bit-reproducible
        if (slab != nullptr) slab[(long)blockIdx.x * 640 + i] = v;
        else if (t < 9) atomicAdd(dw + t * 64 + c, v);
        else atomicAdd(db + c, v);
    }
}

// Backward over the same tile.  Cout == 64: 8 channel groups x 32 pixel lanes, pixel lane pl takes the run's pixels pl, pl + 32, ... in order.
// Routing without a lookup (LOOKUP == false, shipped): the gradient of a pooled output goes to window element `best`, i.e. tap t multiplies
// patch[(best >> 1) + t / 3][(best & 1) + t % 3].  Instead of addressing the patch per channel, g_e = (best == e) ? gv : 0 for the four elements
// and ALL 4 x 9 fused multiply-adds are issued per channel pair on the register-held patch: fma(p, 0, acc) == acc for finite p (acc is never
// -0), so each accumulator sees the one effective fma per pixel the first generation made, bit for bit — 144 v_pk_fma_f32 and no LDS traffic
// beyond the 16 broadcast reads of the patch, against 72 data-dependent LDS reads + 36 v_pk_fma_f32 (LOOKUP == true, experiments flavour,
// OCR_CONV1_LOOKUP=1: the taps straight from the shared tile — 19.0 us against 17.3 at 64 x 256 x 32, 24.9 against 22.1 at 64 x 320 x 32,
// profiles/r12_conv1_kernels.log).
template <bool CODES /* routing + ReLU bits from the forward pass: no window recomputation */, bool LOOKUP>
__global__ __launch_bounds__(256) void conv1_pool_bwd_tile_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                  const bf16_t* __restrict__ dp, float* __restrict__ dw, float* __restrict__ db, int Nb,
                                                                  int W, int H, int pix_per_block, unsigned rH, unsigned rHo, unsigned rWo,
                                                                  const uint32_t* __restrict__ codes, float* __restrict__ slab) {
    extern __shared__ float conv1_tile[];
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const int gq = threadIdx.x & 7, pl = threadIdx.x >> 3;
    float wr[CODES ? 1 : 9][8], br[8];
    if (!CODES) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) wr[CODES ? 0 : t][c] = w[t * 64 + gq * 8 + c];
#pragma unroll
        for (int c = 0; c < 8; ++c) br[c] = bias[gq * 8 + c];
    }
    const unsigned npix = (unsigned)Nb * (W >> 1) * (H >> 1);                       // < 2^31 (checked by the host); the grid is ceil(npix / ppb) >= 1 blocks
    const unsigned p0 = blockIdx.x * (unsigned)pix_per_block, p1 = min(npix, p0 + (unsigned)pix_per_block);
    f32x2 acc2[10][4];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc2[t][q] = (f32x2){0.f, 0.f};
    const Conv1Geo geo = conv1_tile_stage(x, Nb, W, H, p0, p1, rH, rHo, rWo, conv1_tile);
    for (unsigned i = pl; i < p1 - p0; i += 32) {
        const long op = (long)p0 + i;
        float patch[4][4];
        uint32_t word = 0;
        const Conv1Pix px = conv1_tile_pixel(conv1_tile, geo, i);
        conv1_tile_patch(px, geo.RS, patch);
        if constexpr (CODES) {
            word = codes[op * 8 + gq];
        } else {                        // the forward pass's arithmetic on the same values: the same codes
            float o[4][8];
            u32x4 pk;
            conv1_window_fma(patch, wr, br, o);
            word = conv1_pool_pack(o, pk);
        }
        float g[8];
        unpack8(*(const u32x4*)(dp + op * 64 + gq * 8), g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c0 = (int)((word >> (8 * q)) & 7u), c1 = (int)((word >> (8 * q + 4)) & 7u);
            const f32x2 gv = {(c0 & 4) ? g[2 * q] : 0.f, (c1 & 4) ? g[2 * q + 1] : 0.f};        // ReLU mask of the winning element
            acc2[9][q] += gv;
            if constexpr (LOOKUP) {
                const int a0 = c0 >> 1 & 1, a1 = c1 >> 1 & 1;
                const float* t0 = px.base + a0 * geo.RS + (c0 & 1);
                const float* t1 = px.base + a1 * geo.RS + (c1 & 1);
                // patch row a + t / 3: row 0 (a == 0, first tap row) and row 3 (a == 1, last tap row) read as zero at an image's edge
                const bool zt0 = px.top && !a0, zb0 = px.bottom && a0, zt1 = px.top && !a1, zb1 = px.bottom && a1;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    f32x2 xv = {t0[(t / 3) * geo.RS + t % 3], t1[(t / 3) * geo.RS + t % 3]};
                    if (t / 3 == 0) xv = (f32x2){zt0 ? 0.f : xv.x, zt1 ? 0.f : xv.y};
                    if (t / 3 == 2) xv = (f32x2){zb0 ? 0.f : xv.x, zb1 ? 0.f : xv.y};
                    acc2[t][q] = __builtin_elementwise_fma(xv, gv, acc2[t][q]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f32x2 ge = {(c0 & 3) == e ? gv.x : 0.f, (c1 & 3) == e ? gv.y : 0.f};
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        const float pv = patch[(e >> 1) + t / 3][(e & 1) + t % 3];
                        acc2[t][q] = __builtin_elementwise_fma((f32x2){pv, pv}, ge, acc2[t][q]);
                    }
                }
            }
        }
    }
    float acc[10][8];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) { acc[t][2 * q] = acc2[t][q].x; acc[t][2 * q + 1] = acc2[t][q].y; }
    conv1_bwd_reduce(acc, dw, db, slab);
}


// ============================================================================================
// max-pool (VALID, window == stride, kw over axis W in {1,2}, kh over axis H in {1,2})
//   reference: Network.max_pool  network.py:343-350 ; LSTM_train.py:25,27,30,33
// ============================================================================================
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

template <int KW, int KH>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                          int Nb, int W, int H, int C) {
    constexpr int kw = KW, kh = KH;
    const int Wo = W / kw, Ho = H / kh, groups = C >> 3;
    const long total = (long)Nb * Wo * Ho * groups;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        int gq = (int)(idx % groups);
        long op = idx / groups;
        int ho = (int)(op % Ho);
        long q = op / Ho;
        int wo = (int)(q % Wo);
        long n = q / Wo;
        const bf16_t* base = x + (((n * W + (long)wo * kw) * H) + (long)ho * kh) * C + gq * 8;
        u32x4 m = *(const u32x4*)base;
#pragma unroll
        for (int a = 0; a < kw; ++a)
#pragma unroll
            for (int b = 0; b < kh; ++b) {
                if (a == 0 && b == 0) continue;
                m = max8(m, *(const u32x4*)(base + ((long)a * H + b) * C));
            }
        *(u32x4*)(y + op * C + gq * 8) = m;
    }
}

// dx[pixel] = dy[window's output] if this pixel is the FIRST maximum of its window in TF scan order
// (axis W outer, axis H inner), else 0; optionally multiplied by the ReLU mask (x > 0) so the
// result is the gradient w.r.t. the pre-activation of the conv that produced x.
template <int KW, int KH>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                          bf16_t* __restrict__ dx, int Nb, int W, int H, int C,
                                                          int relu_mask) {
    constexpr int kw = KW, kh = KH, cnt_all = KW * KH;
    const int Wo = W / kw, Ho = H / kh, groups = C >> 3;
    const long total = (long)Nb * Wo * Ho * groups;   // one thread per output window x channel group
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        int gq = (int)(idx % groups);
        long op = idx / groups;
        int ho = (int)(op % Ho);
        long q = op / Ho;
        int wo = (int)(q % Wo);
        long n = q / Wo;
        long boff = (((n * W + (long)wo * kw) * H) + (long)ho * kh) * C + gq * 8;
        float xv[cnt_all][8];
#pragma unroll
        for (int a = 0; a < kw; ++a)
#pragma unroll
            for (int b = 0; b < kh; ++b) {
                u32x4 v = *(const u32x4*)(x + boff + ((long)a * H + b) * C);
                unpack8(v, xv[a * kh + b]);
            }
        float g[8];
        unpack8(*(const u32x4*)(dy + op * C + gq * 8), g);
        int win[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            int best = 0; float bv = xv[0][c];
#pragma unroll
            for (int e = 1; e < cnt_all; ++e) if (xv[e][c] > bv) { bv = xv[e][c]; best = e; }
            win[c] = best;
        }
#pragma unroll
        for (int a = 0; a < kw; ++a)
#pragma unroll
            for (int b = 0; b < kh; ++b) {
                const int cnt = a * kh + b;
                float o[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    float v = (win[c] == cnt) ? g[c] : 0.f;
                    if (relu_mask && !(xv[cnt][c] > 0.f)) v = 0.f;
                    o[c] = v;
                }
                u32x4 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
                *(u32x4*)(dx + boff + ((long)a * H + b) * C) = pk;
            }
    }
}

// maxpool_bwd_kernel from the routing codes the forward pass saved (codes[window][C / 8], common.h's pool_code_word) instead of the full-resolution
// tensor: the same thread layout, the same decisions (first maximum; relu_mask: the winner's value > 0 = bit 2), bit-identical dx.
template <int KW, int KH>
__global__ __launch_bounds__(256) void maxpool_bwd_codes_kernel(const uint32_t* __restrict__ codes, const bf16_t* __restrict__ dy,
                                                                bf16_t* __restrict__ dx, int Nb, int W, int H, int C,
                                                                int relu_mask) {
    constexpr int kw = KW, kh = KH;
    const int Wo = W / kw, Ho = H / kh, groups = C >> 3;
    const long total = (long)Nb * Wo * Ho * groups;   // one thread per output window x channel group
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        int gq = (int)(idx % groups);
        long op = idx / groups;
        int ho = (int)(op % Ho);
        long q = op / Ho;
        int wo = (int)(q % Wo);
        long n = q / Wo;
        long boff = (((n * W + (long)wo * kw) * H) + (long)ho * kh) * C + gq * 8;
        const uint32_t word = codes[idx];
        float g[8];
        unpack8(*(const u32x4*)(dy + op * C + gq * 8), g);
        if (relu_mask) {
#pragma unroll
            for (int c = 0; c < 8; ++c) if (!((word >> (4 * c)) & 4u)) g[c] = 0.f;
        }
#pragma unroll
        for (int a = 0; a < kw; ++a)
#pragma unroll
            for (int b = 0; b < kh; ++b) {
                const int cnt = a * kh + b;
                float o[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) o[c] = (((word >> (4 * c)) & 3u) == (uint32_t)cnt) ? g[c] : 0.f;
                u32x4 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
                *(u32x4*)(dx + boff + ((long)a * H + b) * C) = pk;
            }
    }
}

// ============================================================================================
// training-mode batch norm over rows of x[M][C] (bf16), biased variance, eps (TF contrib default 1e-3)
//   reference: tf.contrib.layers.batch_norm(..., is_training=True)  network.py:176-178  (always batch stats)
// ============================================================================================
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

// Batch statistics are reduced in two stages without atomics or a zeroed accumulator: every block writes its partial sums
// to its own row part[block][2][C] (fp32, <= a few hundred rows each) and a small second kernel adds the rows up in
// double.  (One double atomic per channel per block was 524 k same-address atomics per layer: 20 us for a 17 MB read.)
// rows per block for ~`target` blocks, multiple of 8 (measured on [16384, 512]: forward statistics best with 256 blocks,
// backward statistics — three tensors per row — with 512)
static int bn_rows_per_block_host(long M, int target) {
    long r = (M + target - 1) / target;
    r = (r + 7) / 8 * 8;
    return (int)(r < 8 ? 8 : r);
}
// pass 1: per-channel sum / sum of squares of this block's rows -> part[block][2][C]
__global__ __launch_bounds__(256) void bn_stats_kernel(const bf16_t* __restrict__ x, float* __restrict__ part,
                                                       long M, int C, int rows_per_block) {
    const int groups = C >> 3;                 // threads along channels (<= 256)
    const int rl = threadIdx.x / groups;       // row lane
    const int gq = threadIdx.x % groups;
    const int rlanes = 256 / groups;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float s[8], ss[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { s[c] = 0.f; ss[c] = 0.f; }
    if (rl < rlanes) {
#pragma unroll 4
        for (long r = r0 + rl; r < r1; r += rlanes) {
            float v[8];
            unpack8(*(const u32x4*)(x + r * C + gq * 8), v);
#pragma unroll
            for (int c = 0; c < 8; ++c) { s[c] += v[c]; ss[c] = fmaf(v[c], v[c], ss[c]); }
        }
    }
    __shared__ float red[2048];
    float* dst = part + (long)blockIdx.x * 2 * C;
    block_channel_reduce<float, true>(s, red, dst, C, groups, rl, gq, rlanes);
    block_channel_reduce<float, true>(ss, red, dst + C, C, groups, rl, gq, rlanes);
}
// Column sums of part[nblk][2C] for the channel pair (c, C + c): 256 threads = 16 channels x 16 row lanes, every lane adds
// nblk/16 rows in double (independent loads), then the 16 lanes of a channel meet in LDS.  Returns the totals to row lane 0.
__device__ __forceinline__ bool bn_pair_sum(const float* __restrict__ part, int nblk, int C, double& t0, double& t1, int& ch) {
    __shared__ double red[2][16][17];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    ch = blockIdx.x * 16 + cl;
    double a0 = 0, a1 = 0;
    if (ch < C) {
#pragma unroll 4
        for (int b = rl; b < nblk; b += 16) {
            a0 += (double)part[(long)b * 2 * C + ch];
            a1 += (double)part[(long)b * 2 * C + C + ch];
        }
    }
    red[0][rl][cl] = a0; red[1][rl][cl] = a1;
    __syncthreads();
    if (rl != 0 || ch >= C) return false;
    t0 = 0; t1 = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) { t0 += red[0][r][cl]; t1 += red[1][r][cl]; }
    return true;
}
// pass 2 (tiny): mean / rstd
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ part, int nblk, float* __restrict__ mean,
                                                          float* __restrict__ rstd, long M, int C, float eps) {
    double s, ss; int c;
    if (bn_pair_sum(part, nblk, C, s, ss, c)) {
        double mu = s / (double)M;
        double var = ss / (double)M - mu * mu;
        if (var < 0) var = 0;
        mean[c] = (float)mu;
        rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    }
}
// pass 3: y = [relu](gamma * (x - mean) * rstd + beta).  A thread keeps ONE 8-channel group (its scale / shift live in
// registers) and walks rows: the first version re-loaded 32 per-channel parameters for every 16 bytes of data.
__global__ __launch_bounds__(256) void bn_apply_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       long M, int C, int relu, int rows_per_block, const bf16_t* __restrict__ res) {
    const int groups = C >> 3;
    const int rl = threadIdx.x / groups, gq = threadIdx.x % groups, rlanes = 256 / groups;
    if (rl >= rlanes) return;
    float mu[8], rs[8], gm[8], bt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ch = gq * 8 + c;
        mu[c] = mean[ch]; rs[c] = rstd[ch]; gm[c] = gamma[ch]; bt[c] = beta[ch];
    }
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
#pragma unroll 4
    for (long r = r0 + rl; r < r1; r += rlanes) {
        float v[8], o[8];
        unpack8(*(const u32x4*)(x + r * C + gq * 8), v);
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = (v[c] - mu[c]) * rs[c] * gm[c] + bt[c];
        if (res != nullptr) {
            // residual block tail in the same pass: y = [relu](bf16(bn) + res) — the batch-norm output is rounded to bf16 first, so the
            // result is bit-identical to batch-norm, add and relu as three passes (Network.add / Network.relu, network.py:340,461)
            float q[8];
            unpack8(*(const u32x4*)(res + r * C + gq * 8), q);
            u32x4 rb = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
            unpack8(rb, o);
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] += q[c];
        }
        if (relu) {
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] = fmaxf(o[c], 0.f);
        }
        u32x4 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
        *(u32x4*)(y + r * C + gq * 8) = pk;
    }
}
// pass 3 with the max-pool that follows the layer (LSTM_train.py:33: conv4_2 -> max_pool 1 x 2 over the feature axis = row pairs (2q, 2q + 1)
// of the [M][C] view): y is written as by bn_apply_kernel (the backward pass needs it) AND pooled[q] = max(y[2q], y[2q + 1]) — bf16 max of the
// rounded values, i.e. bit-identical to maxpool_fwd_kernel<1, 2> on the stored tensor.  A thread keeps one channel group and walks PAIRS.
// codes != NULL (training): the pair's routing codes (pool_code_word: which row is the first maximum, maximum > 0) are written INSTEAD of y —
// all that the backward passes take from y when this pool is the layer's only consumer (bn_pool_route_codes).
__global__ __launch_bounds__(256) void bn_apply_pool_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, bf16_t* __restrict__ pooled,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            long M, int C, int relu, int pairs_per_block, uint32_t* __restrict__ codes) {
    const int groups = C >> 3;
    const int rl = threadIdx.x / groups, gq = threadIdx.x % groups, rlanes = 256 / groups;
    if (rl >= rlanes) return;
    float mu[8], rs[8], gm[8], bt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ch = gq * 8 + c;
        mu[c] = mean[ch]; rs[c] = rstd[ch]; gm[c] = gamma[ch]; bt[c] = beta[ch];
    }
    const long q0 = (long)blockIdx.x * pairs_per_block, q1 = min(M >> 1, q0 + pairs_per_block);
#pragma unroll 2
    for (long q = q0 + rl; q < q1; q += rlanes) {
        u32x4 pk[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float v[8], o[8];
            unpack8(*(const u32x4*)(x + (2 * q + e) * C + gq * 8), v);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                o[c] = (v[c] - mu[c]) * rs[c] * gm[c] + bt[c];
                if (relu) o[c] = fmaxf(o[c], 0.f);
            }
            pk[e] = (u32x4){pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
            if (codes == nullptr) *(u32x4*)(y + (2 * q + e) * C + gq * 8) = pk[e];
        }
        *(u32x4*)(pooled + q * C + gq * 8) = max8(pk[0], pk[1]);
        if (codes != nullptr) codes[q * groups + gq] = pool_code_word(pk);
    }
}
// The gradient of row r when the layer's consumer is that 1 x 2 max-pool and dy holds the POOLED gradient [M / 2][C]: the pool routes
// dp[r / 2] to the FIRST maximum of the pair (maxpool_bwd_kernel: row 2q + 1 wins only if y[2q + 1] > y[2q]); the ReLU mask follows as usual.
__device__ __forceinline__ void bn_pool_route(const bf16_t* __restrict__ y, const bf16_t* __restrict__ dp, long r, int C, int gq,
                                              const float (&yv)[8], float (&g)[8]) {
    float other[8];
    unpack8(*(const u32x4*)(y + (r ^ 1) * C + gq * 8), other);
    unpack8(*(const u32x4*)(dp + (r >> 1) * C + gq * 8), g);
    const bool odd = (r & 1) != 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool win = odd ? (yv[c] > other[c]) : !(other[c] > yv[c]);
        if (!win) g[c] = 0.f;
    }
}
// ... from the codes bn_apply_pool_kernel saved: one word instead of two rows of y.  Bit 0 names the winning row of the pair, bit 2 is the
// ReLU mask of the winner (a losing row's gradient is zero whatever its own mask says): the decisions bn_pool_route + (y > 0) take on y.
__device__ __forceinline__ void bn_pool_mask_codes(uint32_t word, long r, int relu, float (&g)[8]) {
    const uint32_t odd = (uint32_t)(r & 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t code = word >> (4 * c);
        if ((code & 1u) != odd || (relu && !(code & 4u))) g[c] = 0.f;
    }
}
__device__ __forceinline__ void bn_pool_route_codes(const uint32_t* __restrict__ codes, const bf16_t* __restrict__ dp, long r, int C, int gq,
                                                    int relu, float (&g)[8]) {
    const uint32_t word = codes[(r >> 1) * (C >> 3) + gq];
    unpack8(*(const u32x4*)(dp + (r >> 1) * C + gq * 8), g);
    bn_pool_mask_codes(word, r, relu, g);
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
// backward pass 1: dz = dy * (y > 0) [if relu]; part[block][0][C] = sum dz, part[block][1][C] = sum dz * xhat over the block's rows
// CODES (both backward passes): the pooled gradient is routed and masked from the forward pass's codes, y is not read — instances of their own:
// as a run-time branch of the common kernels it cost the 35 small layers of the ResNet configuration 0.3-0.4 us per launch.
template <bool CODES>
__global__ __launch_bounds__(256) void bn_bwd_stats_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ y,
                                                           const bf16_t* __restrict__ dy, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float* __restrict__ part,
                                                           long M, int C, int rows_per_block, int relu, int pooled,
                                                           const uint32_t* __restrict__ codes) {
    const int groups = C >> 3;
    const int rl = threadIdx.x / groups, gq = threadIdx.x % groups, rlanes = 256 / groups;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float s[8], sx[8], mu[8], rs[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { s[c] = 0.f; sx[c] = 0.f; mu[c] = mean[gq * 8 + c]; rs[c] = rstd[gq * 8 + c]; }
    if (rl < rlanes) {
#pragma unroll 4
        for (long r = r0 + rl; r < r1; r += rlanes) {
            float xv[8], yv[8], g[8];
            unpack8(*(const u32x4*)(x + r * C + gq * 8), xv);
            if constexpr (CODES) bn_pool_route_codes(codes, dy, r, C, gq, relu, g);       // routes and masks: y is not read
            else {
                if (relu || pooled) unpack8(*(const u32x4*)(y + r * C + gq * 8), yv);
                if (pooled) bn_pool_route(y, dy, r, C, gq, yv, g);        // dy = the pooled gradient [M / 2][C]
                else unpack8(*(const u32x4*)(dy + r * C + gq * 8), g);
                if (relu) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) if (!(yv[c] > 0.f)) g[c] = 0.f;
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) { s[c] += g[c]; sx[c] = fmaf(g[c], (xv[c] - mu[c]) * rs[c], sx[c]); }
        }
    }
    __shared__ float red[2048];
    float* dst = part + (long)blockIdx.x * 2 * C;
    block_channel_reduce<float, true>(s, red, dst, C, groups, rl, gq, rlanes);
    block_channel_reduce<float, true>(sx, red, dst + C, C, groups, rl, gq, rlanes);
}
// bn_bwd_stats_kernel<true> with conv5's col2im inside: the pooled gradient of pair q = r >> 1 is formed from the column matrix (col2im_unit8:
// two independent 16-byte loads where the plain kernel has one, in an iteration that waits on loads anyway) instead of read from a tensor
// that a launch of its own wrote and this one re-read; the thread of the pair's EVEN row stores it to dyp for the apply pass.  Rows per block,
// thread-to-row mapping, accumulation order and the reduction are the plain kernel's: the same partial rows, bit for bit.
__global__ __launch_bounds__(256) void bn_bwd_stats_col_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ col, int W, int HC,
                                                               bf16_t* __restrict__ dyp, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ part,
                                                               long M, int C, int rows_per_block, int relu,
                                                               const uint32_t* __restrict__ codes) {
    const int groups = C >> 3;
    const int rl = threadIdx.x / groups, gq = threadIdx.x % groups, rlanes = 256 / groups;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float s[8], sx[8], mu[8], rs[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { s[c] = 0.f; sx[c] = 0.f; mu[c] = mean[gq * 8 + c]; rs[c] = rstd[gq * 8 + c]; }
    if (rl < rlanes) {
#pragma unroll 4
        for (long r = r0 + rl; r < r1; r += rlanes) {
            float xv[8], g[8];
            unpack8(*(const u32x4*)(x + r * C + gq * 8), xv);
            const long q = r >> 1;
            const uint32_t word = codes[q * groups + gq];
            const u32x4 pk = col2im_unit8(col, (unsigned)(q * groups + gq), W, HC);        // < 2^31 units (checked by the host)
            if (!(r & 1)) *(u32x4*)(dyp + q * C + gq * 8) = pk;
            unpack8(pk, g);
            bn_pool_mask_codes(word, r, relu, g);
#pragma unroll
            for (int c = 0; c < 8; ++c) { s[c] += g[c]; sx[c] = fmaf(g[c], (xv[c] - mu[c]) * rs[c], sx[c]); }
        }
    }
    __shared__ float red[2048];
    float* dst = part + (long)blockIdx.x * 2 * C;
    block_channel_reduce<float, true>(s, red, dst, C, groups, rl, gq, rlanes);
    block_channel_reduce<float, true>(sx, red, dst + C, C, groups, rl, gq, rlanes);
}
// backward pass 1b (tiny): sums[2][C] (double) = column sums of the partial rows; dbeta += sum dz, dgamma += sum dz * xhat
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ part, int nblk, double* __restrict__ sums,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, int C) {
    double s, sx; int c;
    if (bn_pair_sum(part, nblk, C, s, sx, c)) {
        sums[c] = s; sums[C + c] = sx;
        dbeta[c] += (float)s;
        dgamma[c] += (float)sx;
    }
}
// backward pass 2: dx = gamma*rstd*(dz - mean(dz) - xhat*mean(dz*xhat))   (per-thread channel group, as bn_apply_kernel)
template <bool CODES>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ y,
                                                           const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const double* __restrict__ sums,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           long M, int C, int relu, int rows_per_block, int pooled,
                                                           const uint32_t* __restrict__ codes) {
    const int groups = C >> 3;
    const int rl = threadIdx.x / groups, gq = threadIdx.x % groups, rlanes = 256 / groups;
    if (rl >= rlanes) return;
    const double invM = 1.0 / (double)M;
    float mu[8], rs[8], gr[8], mdz[8], mdzx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ch = gq * 8 + c;
        mu[c] = mean[ch]; rs[c] = rstd[ch]; gr[c] = gamma[ch] * rstd[ch];
        mdz[c] = (float)(sums[ch] * invM); mdzx[c] = (float)(sums[C + ch] * invM);
    }
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
#pragma unroll 2
    for (long r = r0 + rl; r < r1; r += rlanes) {
        float xv[8], yv[8], g[8], o[8];
        unpack8(*(const u32x4*)(x + r * C + gq * 8), xv);
        if constexpr (CODES) bn_pool_route_codes(codes, dy, r, C, gq, relu, g);
        else {
            if (relu || pooled) unpack8(*(const u32x4*)(y + r * C + gq * 8), yv);
            if (pooled) bn_pool_route(y, dy, r, C, gq, yv, g);
            else unpack8(*(const u32x4*)(dy + r * C + gq * 8), g);
            if (relu) {
#pragma unroll
                for (int c = 0; c < 8; ++c) if (!(yv[c] > 0.f)) g[c] = 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float xh = (xv[c] - mu[c]) * rs[c];
            o[c] = gr[c] * (g[c] - mdz[c] - xh * mdzx[c]);
        }
        u32x4 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
        *(u32x4*)(dx + r * C + gq * 8) = pk;
    }
}

#ifdef OCR_EXPERIMENTS
// ---- fused batch-norm passes (round 3, MEASURED AND REJECTED — experiments build only, OCR_BN_FUSED=1): ONE launch per pass.
// Result (profiles/r03z_bn_fused.log): correct (engine and golden tests pass), but a grid barrier across the 8 XCDs costs 10-20 us (one
// counter: ~20, two-level: ~10; device-scope atomics and the L2 write-back / invalidate of the release / acquire fences), so a fused pass
// takes ~41 us against ~25 for the three launches it replaces: the headline step 1.333 -> 1.397 ms, the deep one 5.27 -> 6.54 ms.  The three-kernel forms above read x twice (x, y and dy twice in the backward
// pass) and pay three dependent launches of 5-14 us for 17 MB tensors: 2 x (19 + 33) us per step of the headline net, 6 launches per
// layer-pass of the 35 BN layers of the deep one.  Here the whole tensor stays in REGISTERS between the statistics and the apply phase
// (<= 256 workgroups x 256 threads x 16 rows x 8 channels = 8.4 M elements: every BN layer of both nets), the per-block partial sums
// meet through two grid barriers: phase 1 block partials -> barrier -> phase 2 block b finalises channels b, b + NB, .. (fixed order,
// double) -> barrier -> phase 3 apply from registers.  All workgroups of the grid are co-resident by construction (<= 256 workgroups of
// 256 threads); the barrier spins on a generation word with a bounded wait (a time-out poisons the output instead of hanging the GPU).
// Two-level barrier: 16 groups (block & 15) count on their own 128-byte lines, the last block of a group counts on the global line, the
// last group releases 16 generation words (one per group, polled by its <= 16 members).  (One counter for all 256 blocks serialised 256
// same-address device-scope atomics: ~20 us per barrier, a fused pass 64 us.)
struct BnBar { unsigned cnt[16][32]; unsigned gen[16][32]; unsigned gcnt[32]; unsigned timeouts[32]; };
__device__ BnBar bn_bar;
__device__ __forceinline__ bool bn_grid_barrier(unsigned nblocks) {
    __syncthreads();                                   // every thread's global stores have been issued and counted (workgroup scope)
    __shared__ int ok_s;
    if (threadIdx.x == 0) {
        int ok = 1;
        __threadfence();                               // release at agent scope ONCE per block (a fence per thread — 65 536 L2 write-backs
                                                       // and invalidates — made a pass 93 us)
        const unsigned g = blockIdx.x & 15u, ngroups = nblocks < 16u ? nblocks : 16u, ng = (nblocks - g + 15u) >> 4;
        const unsigned gen = __hip_atomic_load(&bn_bar.gen[g][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned prev = __hip_atomic_fetch_add(&bn_bar.cnt[g][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool released = false;
        if (prev == ng - 1) {
            __hip_atomic_store(&bn_bar.cnt[g][0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned gp = __hip_atomic_fetch_add(&bn_bar.gcnt[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (gp == ngroups - 1) {
                __hip_atomic_store(&bn_bar.gcnt[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (unsigned k = 0; k < ngroups; ++k) __hip_atomic_store(&bn_bar.gen[k][0], gen + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                released = true;
            }
        }
        if (!released) {
            long spins = 0;
            while (__hip_atomic_load(&bn_bar.gen[g][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > (1L << 22)) { ok = 0; atomicAdd(&bn_bar.timeouts[0], 1u); break; }   // ~ a second: something is badly wrong
            }
        }
        __threadfence();                               // acquire: the other blocks' writes (invalidates this XCD's view)
        ok_s = ok;
    }
    __syncthreads();
    return ok_s != 0;
}
// rows of a block: rows_per_block = NIT_MAX * rlanes at most; thread (rl, gq) owns rows r0 + rl + i * rlanes, channels gq*8 .. gq*8+7
constexpr int BNF_NIT = 16;
// this block's share of the finalisation: channel ch (block-uniform); 256 threads add the NB partial rows of the pair (ch, C + ch) in double
__device__ __forceinline__ void bnf_pair_total(const float* __restrict__ part, int nblk, int C, int ch, double* red /* [2][256] */, double& t0, double& t1) {
    double a0 = 0, a1 = 0;
    for (int b = threadIdx.x; b < nblk; b += 256) { a0 += (double)part[(long)b * 2 * C + ch]; a1 += (double)part[(long)b * 2 * C + C + ch]; }
    red[threadIdx.x] = a0; red[256 + threadIdx.x] = a1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { red[threadIdx.x] += red[threadIdx.x + s]; red[256 + threadIdx.x] += red[256 + threadIdx.x + s]; }
        __syncthreads();
    }
    t0 = red[0]; t1 = red[256];
    __syncthreads();
}
__global__ __launch_bounds__(256) void bn_fused_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ mean, float* __restrict__ rstd,
                                                           float* __restrict__ part, long M, int C, float eps, int relu, int rows_per_block,
                                                           const bf16_t* __restrict__ res) {
    const int groups = C >> 3, rl = threadIdx.x / groups, gq = threadIdx.x % groups, rlanes = 256 / groups;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    const bool act = rl < rlanes;
    u32x4 v[BNF_NIT];
    float s[8], ss[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { s[c] = 0.f; ss[c] = 0.f; }
#pragma unroll
    for (int i = 0; i < BNF_NIT; ++i) {
        const long r = r0 + rl + (long)i * rlanes;
        v[i] = (u32x4){0, 0, 0, 0};
        if (act && r < r1) v[i] = *(const u32x4*)(x + r * C + gq * 8);
    }
#pragma unroll
    for (int i = 0; i < BNF_NIT; ++i) {                // rows past r1 are zeros: they add nothing
        float f[8];
        unpack8(v[i], f);
#pragma unroll
        for (int c = 0; c < 8; ++c) { s[c] += f[c]; ss[c] = fmaf(f[c], f[c], ss[c]); }
    }
    __shared__ float red[2048];
    __shared__ double red2[512];
    float* dst = part + (long)blockIdx.x * 2 * C;
    block_channel_reduce<float, true>(s, red, dst, C, groups, rl, gq, rlanes);
    block_channel_reduce<float, true>(ss, red, dst + C, C, groups, rl, gq, rlanes);
    bool ok = bn_grid_barrier(gridDim.x);
    for (int ch = blockIdx.x; ch < C; ch += gridDim.x) {
        double t0, t1;
        bnf_pair_total(part, gridDim.x, C, ch, red2, t0, t1);
        if (threadIdx.x == 0) {
            const double mu = t0 / (double)M;
            double var = t1 / (double)M - mu * mu;
            if (var < 0) var = 0;
            mean[ch] = (float)mu;
            rstd[ch] = (float)(1.0 / sqrt(var + (double)eps));
        }
    }
    ok = bn_grid_barrier(gridDim.x) && ok;
    if (!act) return;
    float mu[8], rs[8], gm[8], bt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ch = gq * 8 + c;
        mu[c] = mean[ch]; rs[c] = ok ? rstd[ch] : __builtin_nanf(""); gm[c] = gamma[ch]; bt[c] = beta[ch];
    }
#pragma unroll
    for (int i = 0; i < BNF_NIT; ++i) {
        const long r = r0 + rl + (long)i * rlanes;
        if (r >= r1) continue;
        float f[8], o[8];
        unpack8(v[i], f);
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = (f[c] - mu[c]) * rs[c] * gm[c] + bt[c];
        if (res != nullptr) {                          // as bn_apply_kernel: the batch-norm output is rounded to bf16 before the add
            float q[8];
            unpack8(*(const u32x4*)(res + r * C + gq * 8), q);
            u32x4 rb = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
            unpack8(rb, o);
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] += q[c];
        }
        if (relu) {
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] = fmaxf(o[c], 0.f);
        }
        u32x4 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
        *(u32x4*)(y + r * C + gq * 8) = pk;
    }
}
__global__ __launch_bounds__(256) void bn_fused_bwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ y, const bf16_t* __restrict__ dy,
                                                           bf16_t* __restrict__ dx, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, float* __restrict__ part, double* __restrict__ sums,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, long M, int C, int relu,
                                                           int rows_per_block) {
    const int groups = C >> 3, rl = threadIdx.x / groups, gq = threadIdx.x % groups, rlanes = 256 / groups;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    const bool act = rl < rlanes;
    u32x4 vx[BNF_NIT], vg[BNF_NIT];
    float s[8], sx[8], mu[8], rs[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { s[c] = 0.f; sx[c] = 0.f; mu[c] = mean[gq * 8 + c]; rs[c] = rstd[gq * 8 + c]; }
#pragma unroll
    for (int i = 0; i < BNF_NIT; ++i) {
        const long r = r0 + rl + (long)i * rlanes;
        vx[i] = (u32x4){0, 0, 0, 0}; vg[i] = (u32x4){0, 0, 0, 0};
        if (act && r < r1) {
            vx[i] = *(const u32x4*)(x + r * C + gq * 8);
            u32x4 g = *(const u32x4*)(dy + r * C + gq * 8);
            if (relu) {                                // dz = dy * (y > 0): cleared halves are exact zeros
                const u32x4 q = *(const u32x4*)(y + r * C + gq * 8);
                if (!(bf_lo(q.x) > 0.f)) g.x &= 0xffff0000u;
                if (!(bf_hi(q.x) > 0.f)) g.x &= 0x0000ffffu;
                if (!(bf_lo(q.y) > 0.f)) g.y &= 0xffff0000u;
                if (!(bf_hi(q.y) > 0.f)) g.y &= 0x0000ffffu;
                if (!(bf_lo(q.z) > 0.f)) g.z &= 0xffff0000u;
                if (!(bf_hi(q.z) > 0.f)) g.z &= 0x0000ffffu;
                if (!(bf_lo(q.w) > 0.f)) g.w &= 0xffff0000u;
                if (!(bf_hi(q.w) > 0.f)) g.w &= 0x0000ffffu;
            }
            vg[i] = g;
        }
    }
#pragma unroll
    for (int i = 0; i < BNF_NIT; ++i) {                // rows past r1: dz = 0 adds nothing
        float xv[8], g[8];
        unpack8(vx[i], xv); unpack8(vg[i], g);
#pragma unroll
        for (int c = 0; c < 8; ++c) { s[c] += g[c]; sx[c] = fmaf(g[c], (xv[c] - mu[c]) * rs[c], sx[c]); }
    }
    __shared__ float red[2048];
    __shared__ double red2[512];
    float* dst = part + (long)blockIdx.x * 2 * C;
    block_channel_reduce<float, true>(s, red, dst, C, groups, rl, gq, rlanes);
    block_channel_reduce<float, true>(sx, red, dst + C, C, groups, rl, gq, rlanes);
    bool ok = bn_grid_barrier(gridDim.x);
    for (int ch = blockIdx.x; ch < C; ch += gridDim.x) {
        double t0, t1;
        bnf_pair_total(part, gridDim.x, C, ch, red2, t0, t1);
        if (threadIdx.x == 0) {
            sums[ch] = t0; sums[C + ch] = t1;
            dbeta[ch] += (float)t0;
            dgamma[ch] += (float)t1;
        }
    }
    ok = bn_grid_barrier(gridDim.x) && ok;
    if (!act) return;
    const double invM = 1.0 / (double)M;
    float gr[8], mdz[8], mdzx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ch = gq * 8 + c;
        gr[c] = ok ? gamma[ch] * rs[c] : __builtin_nanf("");
        mdz[c] = (float)(sums[ch] * invM); mdzx[c] = (float)(sums[C + ch] * invM);
    }
#pragma unroll
    for (int i = 0; i < BNF_NIT; ++i) {
        const long r = r0 + rl + (long)i * rlanes;
        if (r >= r1) continue;
        float xv[8], g[8], o[8];
        unpack8(vx[i], xv); unpack8(vg[i], g);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float xh = (xv[c] - mu[c]) * rs[c];
            o[c] = gr[c] * (g[c] - mdz[c] - xh * mdzx[c]);
        }
        u32x4 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
        *(u32x4*)(dx + r * C + gq * 8) = pk;
    }
}
// launch geometry of the fused passes; 0 blocks = not covered (the three-kernel form runs)
static int bnf_blocks(long M, int C, int* rows_per_block) {
    static int on = -1;                         // A/B knob OCR_BN_FUSED = 1 (default 0: the three-kernel passes)
    if (on < 0) { const char* e = getenv("OCR_BN_FUSED"); on = e ? atoi(e) : 0; }
    const int groups = C >> 3;
    if (!on || groups < 1 || groups > 256) return 0;
    const int rlanes = 256 / groups;
    long rpb = (M + 255) / 256;                 // at most 256 workgroups
    rpb = (rpb + rlanes - 1) / rlanes * rlanes;
    if (rpb > (long)BNF_NIT * rlanes) return 0; // more than 16 rows per thread: does not fit the registers
    const long nb = (M + rpb - 1) / rpb;
    const long ws_rows = ceil_div(M, (long)bn_rows_per_block_host(M, 512));      // what ocr_bn_workspace_bytes sized the partial rows for
    if (nb > 256 || nb > ws_rows) return 0;
    *rows_per_block = (int)rpb;
    return (int)nb;
}
#endif

// ============================================================================================
// column sums: out[c] += sum_m a[m][c]   (bias gradients; a is bf16 [M][C], out fp32)
// ============================================================================================
__global__ __launch_bounds__(256) void colsum_kernel(const bf16_t* __restrict__ a, float* __restrict__ out, long M, int C,
                                                     long lda, int rows_per_block) {
    const int groups = C >> 3;
    const int rl = threadIdx.x / groups, gq = threadIdx.x % groups, rlanes = 256 / groups;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float s[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) s[c] = 0.f;
    if (rl < rlanes) {
#pragma unroll 4
        for (long r = r0 + rl; r < r1; r += rlanes) {
            float v[8];
            unpack8(*(const u32x4*)(a + r * lda + gq * 8), v);
#pragma unroll
            for (int c = 0; c < 8; ++c) s[c] += v[c];
        }
    }
    __shared__ float red[2048];
    block_channel_reduce<float>(s, red, out, C, groups, rl, gq, rlanes);
}

// ============================================================================================
// weight packing (fp32 master in TF layouts -> bf16 K-contiguous operand layouts)
// ============================================================================================
// generic: out[perm(c)][r] (bf16, ld = R) = in[r][c] (f32, [R][Cc]);  perm: TF gate-major column c = g*U + u ->
// packed column (u/16)*64 + g*16 + u%16 (see lstm.hip) when lstm_units > 0, identity otherwise.
__global__ void pack_transpose_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int R, int Cc, long ldin,
                                      int lstm_units) {
    __shared__ float tile[32][33];
    int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 32 x 8
    for (int i = ty; i < 32; i += 8) {
        int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < R && c < Cc) ? in[(long)r * ldin + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        int c = c0 + i, r = r0 + tx;
        if (c < Cc && r < R) {
            int pc = c;
            if (lstm_units > 0) { int gidx = c / lstm_units, u = c % lstm_units; pc = (u >> 4) * 64 + gidx * 16 + (u & 15); }
            out[(long)pc * R + r] = f2bf(tile[tx][i]);
        }
    }
}
// conv 3x3 dgrad operand: out[ci][8 - tap][co] = w[tap][ci][co]   (spatial flip, Cin<->Cout role swap)
__global__ void pack_conv_dgrad_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int Cin, int Cout) {
    long total = 9L * Cin * Cout;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        int co = (int)(idx % Cout);
        long q = idx / Cout;
        int ci = (int)(q % Cin);
        int tap = (int)(q / Cin);
        out[((long)ci * 9 + (8 - tap)) * Cout + co] = f2bf(w[idx]);
    }
}
__global__ void cast_f32_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, long n) {
    long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    long stride = (long)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        f32x4 v = *(const f32x4*)(in + i);
        u32x2 pk = {pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
        *(u32x2*)(out + i) = pk;
    }
    // tail (n % 4) handled by the last thread of the grid-stride pattern
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long t = n & ~3L; t < n; ++t) out[t] = f2bf(in[t]);
}
// strided 2-D cast: out[r][c] (bf16, ld = ldout) = in[r][c] (f32, ld = ldin), cols % 4 == 0
__global__ void cast2d_f32_bf16_kernel(const float* __restrict__ in, long ldin, bf16_t* __restrict__ out, long ldout,
                                       int rows, int cols) {
    const int c4 = cols >> 2;
    long total = (long)rows * c4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        int c = (int)(idx % c4) * 4;
        long r = idx / c4;
        f32x4 v = *(const f32x4*)(in + r * ldin + c);
        u32x2 pk = {pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
        *(u32x2*)(out + r * ldout + c) = pk;
    }
}
// dlogits[T][N][C] f32  ->  [N][T][C] bf16, scaled (CTC gradient hand-off: mean over batch = 1/N)
__global__ void tnc_to_ntc_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int T, int N, int C, float scale) {
    long total = (long)T * N * C;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        int c = (int)(idx % C);
        long q = idx / C;
        int n = (int)(q % N);
        int t = (int)(q / N);
        out[((long)n * T + t) * C + c] = f2bf(in[idx] * scale);
    }
}
// conv5 dgrad overlap-add: dx[n][w][:] = col[n][w][0:HC] + col[n][w-1][HC:2HC]   (col rows exist for w < W-1)
__global__ void conv5_col2im_kernel(const bf16_t* __restrict__ col, bf16_t* __restrict__ dx, int Nb, int W, int HC) {
    long total = (long)Nb * W * HC;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        int e = (int)(idx % HC);
        long q = idx / HC;
        int w = (int)(q % W);
        long n = q / W;
        float v = 0.f;
        if (w < W - 1) v += bf2f(col[((n * (W - 1) + w) * 2L) * HC + e]);
        if (w > 0) v += bf2f(col[((n * (W - 1) + w - 1) * 2L + 1) * HC + e]);
        dx[idx] = f2bf(v);
    }
}

// the same, eight channels (16 bytes) per thread and 32-bit index arithmetic (the scalar kernel moved two bytes per thread behind two
// 64-bit divisions: 1.9 TB/s); element-wise the same two-term sum and the same rounding, hence bit-identical
__global__ __launch_bounds__(256) void conv5_col2im8_kernel(const bf16_t* __restrict__ col, bf16_t* __restrict__ dx, int Nb, int W, int HC) {
    const unsigned total = (unsigned)Nb * W * ((unsigned)HC >> 3);       // < 2^31 (checked by the host)
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const u32x4 pk = col2im_unit8(col, idx, W, HC);
        *(u32x4*)(dx + (long)idx * 8) = pk;
    }
}

// ============================================================================================
// one-launch weight refresh: a table of pack jobs executed by a single grid (the per-tensor pack kernels above cost
// ~4.5 us each as separate launches - 15 of them per step were ~90 us of pure launch latency)
// ============================================================================================
struct PackJob {            // 64 bytes, mirrored by lstm_ctc_ocr_amd/engine.py (numpy structured dtype)
    int type;               // 0 transpose(+lstm perm), 1 conv dgrad flip, 2 strided cast, 3 flat cast, 4 LSTM bias permutation (fp32 -> fp32)
    int R, Cc;              // type 0/2: rows, cols of the fp32 source ; type 1: Cin, Cout ; type 3: unused
    int lstm_units;         // type 0
    long ldin, ldout;       // type 0: ldin ; type 2: ldin, ldout
    const float* src;
    bf16_t* dst;
    long n;                 // type 1/3: element count
    int block_start, nblocks;
};

__global__ __launch_bounds__(256) void pack_jobs_kernel(const PackJob* __restrict__ jobs, int njobs) {
    __shared__ float tile[64][65];
    // which job is this block's?  The last one whose block_start <= blockIdx.x — found by ALL threads at once (thread t looks at jobs t, t + 256, ...;
    // wave maximum, then the four waves' through LDS).  Round 6: the serial scan `while (blockIdx.x >= jobs[j + 1].block_start) ++j` was one dependent
    // L2 round trip per job in front of every block — ~110 of them for the last blocks of configs[4]'s table (its re-pack launch took 151 us at 1.7 TB/s
    // where the headline's 20-job table runs at 5 TB/s).
    __shared__ int jsel[4];
    int j = 0;
    for (int k = threadIdx.x; k < njobs; k += 256)
        if (jobs[k].block_start <= (int)blockIdx.x) j = k;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) j = max(j, __shfl_xor(j, off));
    if ((threadIdx.x & 63) == 0) jsel[threadIdx.x >> 6] = j;
    __syncthreads();
    j = max(max(jsel[0], jsel[1]), max(jsel[2], jsel[3]));
    const PackJob jb = jobs[j];
    const int b = blockIdx.x - jb.block_start;
    if (jb.type == 0) {                                // fp32 [R][ldin] -> bf16 [Cc][R] (transposed), 64 x 64 tiles:
        const int ctiles = (jb.Cc + 63) / 64;          // 16-byte loads along c, 8-byte stores along r
        const int c0 = (b % ctiles) * 64, r0 = (b / ctiles) * 64;
        {
            const int ty = threadIdx.x >> 4, tx = (threadIdx.x & 15) * 4;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int r = r0 + p * 16 + ty, c = c0 + tx;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (r < jb.R) {
                    const float* src = jb.src + (long)r * jb.ldin + c;
                    if (c + 3 < jb.Cc && (jb.ldin & 3) == 0) v = *(const f32x4*)src;
                    else { if (c < jb.Cc) v.x = src[0]; if (c + 1 < jb.Cc) v.y = src[1]; if (c + 2 < jb.Cc) v.z = src[2]; if (c + 3 < jb.Cc) v.w = src[3]; }
                }
                float* trow = &tile[p * 16 + ty][tx];
                trow[0] = v.x; trow[1] = v.y; trow[2] = v.z; trow[3] = v.w;
            }
        }
        __syncthreads();
        {
            const int cy = threadIdx.x >> 4, rq = (threadIdx.x & 15) * 4;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int cl = p * 16 + cy, c = c0 + cl, r = r0 + rq;
                if (c >= jb.Cc || r >= jb.R) continue;
                int pc = c;
                if (jb.lstm_units > 0) { int gidx = c / jb.lstm_units, u = c % jb.lstm_units; pc = (u >> 4) * 64 + gidx * 16 + (u & 15); }
                bf16_t* dst = jb.dst + (long)pc * jb.R + r;
                if (r + 3 < jb.R && (jb.R & 3) == 0) {
                    u32x2 pk = {pack_bf2(tile[rq][cl], tile[rq + 1][cl]), pack_bf2(tile[rq + 2][cl], tile[rq + 3][cl])};
                    *(u32x2*)dst = pk;
                } else {
                    for (int k = 0; k < 4 && r + k < jb.R; ++k) dst[k] = f2bf(tile[rq + k][cl]);
                }
            }
        }
    } else if (jb.type == 1) {
        const int Cin = jb.R, Cout = jb.Cc;            // Cout % 4 == 0: four output channels per thread and iteration
        const int c4 = Cout >> 2;
        const long total = jb.n >> 2;
        for (long idx = (long)b * 256 + threadIdx.x; idx < total; idx += (long)jb.nblocks * 256) {
            const int co = (int)(idx % c4) * 4;
            const long q = idx / c4;
            const int ci = (int)(q % Cin);
            const int tap = (int)(q / Cin);
            f32x4 v = *(const f32x4*)(jb.src + idx * 4);
            u32x2 pk = {pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
            *(u32x2*)(jb.dst + ((long)ci * 9 + (8 - tap)) * Cout + co) = pk;
        }
    } else if (jb.type == 2) {
        const int c4 = jb.Cc >> 2;
        const long total = (long)jb.R * c4;
        for (long idx = (long)b * 256 + threadIdx.x; idx < total; idx += (long)jb.nblocks * 256) {
            int c = (int)(idx % c4) * 4;
            long r = idx / c4;
            f32x4 v = *(const f32x4*)(jb.src + r * jb.ldin + c);
            u32x2 pk = {pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
            *(u32x2*)(jb.dst + r * jb.ldout + c) = pk;
        }
    } else if (jb.type == 4) {
        // LSTM bias of one direction, fp32 [4U] gate-major -> fp32 in the packed gate-column order of the forward operands
        // ((u / 16) * 64 + g * 16 + u % 16, as lstm_pack_bias_kernel); dst is a float address
        float* out = (float*)jb.dst;
        const int U = jb.lstm_units;
        for (long i = (long)b * 256 + threadIdx.x; i < jb.n; i += (long)jb.nblocks * 256) {
            const int g = (int)(i / U), u = (int)(i % U);
            out[(u >> 4) * 64 + g * 16 + (u & 15)] = jb.src[i];
        }
    } else {
        for (long i = ((long)b * 256 + threadIdx.x) * 4; i + 3 < jb.n; i += (long)jb.nblocks * 256 * 4) {
            f32x4 v = *(const f32x4*)(jb.src + i);
            u32x2 pk = {pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
            *(u32x2*)(jb.dst + i) = pk;
        }
    }
}

// ============================================================================================
// element-wise bf16 helpers for residual graphs (Network.add network.py:461-463, Network.relu :340-341)
//   op 0: out = a + b        op 1: out = max(a, 0)        op 2: out = (b > 0) ? a : 0   (ReLU backward: a = dy, b = y)
//   op 3: out = max(a + b, 0)  (residual add + ReLU)        op 4: out += (b > 0) ? a : 0   (ReLU backward accumulated into out)
// ============================================================================================
__global__ __launch_bounds__(256) void eltwise_bf16_kernel(int op, const bf16_t* __restrict__ a, const bf16_t* __restrict__ b,
                                                           bf16_t* __restrict__ out, long n8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        float x[8], y[8], o[8], z[8];
        unpack8(*(const u32x4*)(a + i * 8), x);
        if (op != 1) unpack8(*(const u32x4*)(b + i * 8), y);
        if (op == 4) unpack8(*(const u32x4*)(out + i * 8), z);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (op == 0) o[c] = x[c] + y[c];
            else if (op == 1) o[c] = fmaxf(x[c], 0.f);
            else if (op == 2) o[c] = y[c] > 0.f ? x[c] : 0.f;
            else if (op == 3) o[c] = fmaxf(x[c] + y[c], 0.f);         // = relu(bf16(a + b)): rounding is monotone and keeps the sign
            else o[c] = z[c] + (y[c] > 0.f ? x[c] : 0.f);
        }
        u32x4 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7])};
        *(u32x4*)(out + i * 8) = pk;
    }
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
// A/B knobs, read once.  OCR_CONV1_V2=1: the second generation of the fused conv1 + pool kernels (32-bit index arithmetic, branch-free
// patch loads, next-iteration prefetch).  Measured on MI355X (profiles/r02i_*) and REJECTED as default: forward 19.8 us against 17.3
// (145 registers = 3 waves per SIMD instead of 4), backward 40 us against 38.6 — the first generation's 64-bit divisions and branchy
// loads are hidden by its occupancy.  OCR_COL2IM_V1=1: the scalar col2im (13.3 us against 5.9 for the 16-byte one).
static bool nn_knob(const char* name, int slot) {
    static int v[4] = {-1, -1, -1, -1};
    if (v[slot] < 0) { const char* e = ocr_tune_env(name); v[slot] = (e && atoi(e) != 0) ? 1 : 0; }
    return v[slot] == 1;
}
#ifdef OCR_EXPERIMENTS
static bool conv1_v1() { return !nn_knob("OCR_CONV1_V2", 0); }
// OCR_CONV1_GEN=1: the first generation of the fused conv1 + pool kernels (per-lane patch loads from HBM, 64-bit index arithmetic, float-compare
// codes, a private LDS patch per thread in the backward) in place of the tile kernels — what profiles/r12_conv1_* measure the latter against.
// OCR_CONV1_LOOKUP=1: the tile backward with its taps read from the shared tile at data-dependent offsets instead of the select-and-multiply form.
static bool conv1_gen1() { return nn_knob("OCR_CONV1_GEN", 2); }
static bool conv1_lookup() { return nn_knob("OCR_CONV1_LOOKUP", 3); }
#endif
static bool col2im_v1() { return nn_knob("OCR_COL2IM_V1", 1); }      // product build: always false (ocr_tune_env); the scalar kernel is also the
                                                                     // fallback for HC % 8 != 0 / unaligned buffers, which is how the tests reach it
static inline int grid_for(long total, int cap = 4096) {
    long b = (total + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

extern "C" int ocr_conv1_fwd(const float* x, const float* w, const float* bias, void* y, int Nb, int W, int H,
                             int Cout, int relu, void* stream) {
    if (!x || !w || !bias || !y || (Cout & 7) || Cout > 1024) return OCR_ERR_INVALID;
    if (256 % (Cout >> 3)) return OCR_ERR_INVALID;
    long total = (long)Nb * W * H * (Cout >> 3);
    conv1_fwd_kernel<<<grid_for(total, 2048), 256, 0, (hipStream_t)stream>>>(
        x, w, bias, (bf16_t*)y, Nb, W, H, Cout, relu);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_conv1_wgrad(const float* x, const void* dz, float* dw, float* db, int Nb, int W, int H, int Cout,
                               void* stream) {
    if (!x || !dz || !dw || !db || Cout != 64) return OCR_ERR_INVALID;
    long npix = (long)Nb * W * H;
    int ppb = 1024;
    conv1_wgrad_kernel<<<ceil_div(npix, ppb), 256, 0, (hipStream_t)stream>>>(x, (const bf16_t*)dz, dw, db, Nb, W, H, Cout, ppb);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_eltwise_bf16(int op, const void* a, const void* b, void* out, long n, void* stream) {
    if (!a || !out || (op != 1 && !b) || op < 0 || op > 4 || n <= 0 || (n & 7)) return OCR_ERR_INVALID;
    eltwise_bf16_kernel<<<grid_for(n / 8, 4096), 256, 0, (hipStream_t)stream>>>(op, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out, n / 8);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
// Launch geometry of the tile kernels (conv1_tile_stage): ceil(npix / ppb) blocks (one at least: the forward's fills), the reciprocals of
// conv1_div, and the dynamic LDS of the largest tile a run of ppb pooled pixels can need — it spans at most 2 + (ppb - 1) / Ho pooled columns,
// two input rows each and a halo row either side, H + 2 words a row (4.9 KB at H = 32 and 256 pixels; 33 KB at H = 2 and 1024).  Refused: 2^31
// pooled pixels or more, and shapes whose index products leave 32 bits or whose tile leaves the 160 KB of a CU (H > ~6800: six rows).
struct Conv1Launch { bool ok; int blocks, ppb, lds; unsigned rH, rHo, rWo; };
static unsigned conv1_recip(long d) { return d > 1 ? (unsigned)((0x100000000ull + (unsigned long)d - 1) / (unsigned long)d) : 0u; }
static Conv1Launch conv1_launch(int Nb, int W, int H, int ppb) {
    Conv1Launch L = {};
    if (Nb < 0 || W < 2 || H < 2) return L;
    const long Wo = W / 2, Ho = H / 2, npix = (long)Nb * Wo * Ho;
    const long cols = std::min<long>(2 + (ppb - 1) / Ho, std::max<long>((long)Nb * Wo, 1)), words = (2 * cols + 2) * (H + 2);
    if (npix >= 0x7fffffffL || words * 4 > 160 * 1024) return L;
    if ((Ho + ppb) * Ho >= 0x100000000L || (Wo + cols) * Wo >= 0x100000000L || words * H >= 0x100000000L) return L;
    L.ok = true; L.ppb = ppb; L.blocks = std::max(1, ceil_div(npix, ppb)); L.lds = (int)words * 4;
    L.rH = conv1_recip(H); L.rHo = conv1_recip(Ho); L.rWo = conv1_recip(Wo);
    return L;
}
// pooled pixels per block of the forward: 128 = 1024 blocks at the headline shape; 64 and 256 measured the same within 1 us (a tuning knob:
// experiments flavour, profiles/r12_conv1_kernels.log)
static int conv1_fwd_ppb() {
    static int v = -1;
    if (v < 0) { const char* e = ocr_tune_env("OCR_CONV1_FWD_PPB"); v = e ? atoi(e) : 128; if (v < 32 || v > 1024 || (v & 31)) v = 128; }
    return v;
}
static int conv1_pool_fwd_impl(const float* x, const float* w, const float* bias, void* p, int Nb, int W, int H, int Cout,
                               float* zero, long zero_n, void* codes, void* ones, long ones_n, void* stream) {
    if (!x || !w || !bias || !p || (Cout & 7) || Cout > 1024 || 256 % (Cout >> 3) || (W & 1) || (H & 1)) return OCR_ERR_INVALID;
    if (zero_n < 0 || (zero_n & 3) || (zero_n && (!zero || ((size_t)zero & 15)))) return OCR_ERR_INVALID;
    if (ones_n < 0 || (ones_n & 3) || (ones_n && (!ones || ((size_t)ones & 15)))) return OCR_ERR_INVALID;
    if (codes && (Cout != 64 || ((size_t)codes & 3))) return OCR_ERR_INVALID;            // the routing codes exist for the 64-filter layer the backward kernel handles
    long total = (long)Nb * (W / 2) * (H / 2) * (Cout >> 3);
    const Conv1Launch L = conv1_launch(Nb, W, H, conv1_fwd_ppb());
    if (!L.ok) return OCR_ERR_INVALID;
#ifdef OCR_EXPERIMENTS
    if (!zero_n && !ones_n && !codes && !conv1_v1() && (long)Nb * (W / 2) * (H / 2) < 0x7fffffffL && (long)Nb * W * H < 0x7fffffffL && (long)W * H < 0x7fffffffL)
        conv1_pool_fwd2_kernel<<<grid_for(total, 2048), 256, 0, (hipStream_t)stream>>>(x, w, bias, (bf16_t*)p, Nb, W, H, Cout);
    else if (conv1_gen1()) {
        if (codes) conv1_pool_fwd_kernel<true><<<grid_for(total, 2048), 256, 0, (hipStream_t)stream>>>(x, w, bias, (bf16_t*)p, Nb, W, H, Cout, (f32x4*)zero,
                                                                                                          zero_n / 4, (uint32_t*)codes, (u32x4*)ones, ones_n / 4);
        else conv1_pool_fwd_kernel<false><<<grid_for(total, 2048), 256, 0, (hipStream_t)stream>>>(x, w, bias, (bf16_t*)p, Nb, W, H, Cout, (f32x4*)zero,
                                                                                                 zero_n / 4, nullptr, (u32x4*)ones, ones_n / 4);
    } else
#endif
    if (codes) {
        if (ocr_allow_lds<conv1_pool_fwd_tile_kernel<true>>(L.lds) != hipSuccess) return OCR_ERR_EXEC;
        conv1_pool_fwd_tile_kernel<true><<<L.blocks, 256, L.lds, (hipStream_t)stream>>>(x, w, bias, (bf16_t*)p, Nb, W, H, Cout, L.ppb, L.rH, L.rHo, L.rWo,
                                                                                       (f32x4*)zero, zero_n / 4, (uint32_t*)codes, (u32x4*)ones, ones_n / 4);
    } else {
        if (ocr_allow_lds<conv1_pool_fwd_tile_kernel<false>>(L.lds) != hipSuccess) return OCR_ERR_EXEC;
        conv1_pool_fwd_tile_kernel<false><<<L.blocks, 256, L.lds, (hipStream_t)stream>>>(x, w, bias, (bf16_t*)p, Nb, W, H, Cout, L.ppb, L.rH, L.rHo, L.rWo,
                                                                                        (f32x4*)zero, zero_n / 4, nullptr, (u32x4*)ones, ones_n / 4);
    }
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_conv1_pool_fwd(const float* x, const float* w, const float* bias, void* p, int Nb, int W, int H, int Cout,
                                  void* stream) {
    return conv1_pool_fwd_impl(x, w, bias, p, Nb, W, H, Cout, nullptr, 0, nullptr, nullptr, 0, stream);
}
// The training form of the same launch.  codes (may be NULL; Cout == 64): uint32 [Nb * W/2 * H/2][8] — per pooled output 4 bits, the position
// of the window's first maximum (on the bf16-rounded values, TF scan order) | ReLU bit << 2: ocr_conv1_pool_bwd_codes routes the gradient with
// them instead of recomputing the window.  zero (may be NULL): fp32 [zero_n] cleared by the same launch (zero_n % 4 == 0, 16-byte aligned):
// the flat gradient buffer of the step that begins.  ones (may be NULL): ones_n 32-bit words (% 4 == 0, 16-byte aligned) set to 0xFFFFFFFF by
// the same launch: the hand-off blocks of the step's persistent LSTM launches (ocr_lstm_fwd_seq2 / ocr_lstm_bwd_seq2 with OCR_LSTM_PREPARED).
extern "C" int ocr_conv1_pool_fwd_train(const float* x, const float* w, const float* bias, void* p, int Nb, int W, int H, int Cout,
                                        void* codes, float* zero, long zero_n, void* ones, long ones_n, void* stream) {
    return conv1_pool_fwd_impl(x, w, bias, p, Nb, W, H, Cout, zero, zero_n, codes, ones, ones_n, stream);
}
// pooled pixels per block of the conv1 + pool backward kernel (a thread walks ppb / 32 of them, one memory round trip each).  With atomics
// smaller blocks were slower (profiles/r04k_conv1_ppb_ab.log: 640 same-address atomics per block); the slab form pays 2.5 KB per block instead.
static int conv1_ppb() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("OCR_CONV1_PPB"); v = e ? atoi(e) : 256; if (v < 32 || v > 1024 || (v & 31)) v = 256; }
    return v;
}
#define CONV1_BWD_TILE(CODES, LOOKUP)                                                                                              \
    do {                                                                                                                           \
        if (ocr_allow_lds<conv1_pool_bwd_tile_kernel<CODES, LOOKUP>>(L.lds) != hipSuccess) return OCR_ERR_EXEC;                    \
        conv1_pool_bwd_tile_kernel<CODES, LOOKUP><<<nb, 256, L.lds, (hipStream_t)stream>>>(x, w, bias, g, dw, db, Nb, W, H, ppb,    \
                                                                                            L.rH, L.rHo, L.rWo, cd, slab);         \
    } while (0)
static int conv1_pool_bwd_impl(const float* x, const float* w, const float* bias, const void* dp, float* dw, float* db,
                               int Nb, int W, int H, int Cout, const void* codes, float* slab, void* stream) {
    if (!x || !w || !bias || !dp || (!slab && (!dw || !db)) || Cout != 64 || (W & 1) || (H & 1) || ((size_t)codes & 3)) return OCR_ERR_INVALID;
    long npix = (long)Nb * (W / 2) * (H / 2);
    int ppb = slab ? conv1_ppb() : 256;
    const Conv1Launch L = conv1_launch(Nb, W, H, ppb);
    if (!L.ok) return OCR_ERR_INVALID;
    const bf16_t* g = (const bf16_t*)dp;
    const uint32_t* cd = (const uint32_t*)codes;
    const int nb = ceil_div(npix, ppb);
#ifdef OCR_EXPERIMENTS
    if (!codes && !slab && !conv1_v1() && npix < 0x7fffffffL - 512 && (long)Nb * W * H < 0x7fffffffL)
        conv1_pool_bwd2_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(x, w, bias, g, dw, db, Nb, W, H, Cout, ppb);
    else if (conv1_gen1()) {
        if (codes) conv1_pool_bwd_kernel<true><<<nb, 256, 0, (hipStream_t)stream>>>(x, w, bias, g, dw, db, Nb, W, H, Cout, ppb, cd, slab);
        else conv1_pool_bwd_kernel<false><<<nb, 256, 0, (hipStream_t)stream>>>(x, w, bias, g, dw, db, Nb, W, H, Cout, ppb, nullptr, slab);
    } else if (conv1_lookup()) {
        if (codes) CONV1_BWD_TILE(true, true); else CONV1_BWD_TILE(false, true);
    } else
#endif
    if (codes) CONV1_BWD_TILE(true, false); else CONV1_BWD_TILE(false, false);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_conv1_pool_bwd(const float* x, const float* w, const float* bias, const void* dp, float* dw, float* db,
                                  int Nb, int W, int H, int Cout, void* stream) {
    return conv1_pool_bwd_impl(x, w, bias, dp, dw, db, Nb, W, H, Cout, nullptr, nullptr, stream);
}
// ... with the routing codes ocr_conv1_pool_fwd_train saved: bit-identical gradients, no recomputation of the 2 x 2 windows
extern "C" int ocr_conv1_pool_bwd_codes(const float* x, const float* w, const float* bias, const void* dp, float* dw, float* db,
                                        int Nb, int W, int H, int Cout, const void* codes, void* stream) {
    if (!codes) return OCR_ERR_INVALID;
    return conv1_pool_bwd_impl(x, w, bias, dp, dw, db, Nb, W, H, Cout, codes, nullptr, stream);
}
// Slab form: no atomics — block b leaves its partial sums in slab[b][640] = {dW [9][64] | db [64]} (fp32), rows = ocr_conv1_pool_bwd_slab_rows;
// the caller adds the rows with ocr_wgrad9_reduce_jobs (two jobs: n4 = 144 / 16, slab4 = 160, S = rows — the engine appends them to the merged
// reduction of the 3x3 layers that runs right behind this kernel anyway): bit-reproducible conv1 gradients.  codes may be NULL (recompute).
extern "C" int ocr_conv1_pool_bwd_slab_rows(int Nb, int W, int H) {
    if (Nb <= 0 || W <= 0 || H <= 0 || (W & 1) || (H & 1)) return 0;
    return (int)ceil_div((long)Nb * (W / 2) * (H / 2), (long)conv1_ppb());
}
extern "C" int ocr_conv1_pool_bwd_slab(const float* x, const float* w, const float* bias, const void* dp, int Nb, int W, int H, int Cout,
                                       const void* codes, float* slab, void* stream) {
    if (!slab || ((size_t)slab & 15)) return OCR_ERR_INVALID;
    return conv1_pool_bwd_impl(x, w, bias, dp, nullptr, nullptr, Nb, W, H, Cout, codes, slab, stream);
}
extern "C" int ocr_maxpool_fwd(const void* x, void* y, int Nb, int W, int H, int C, int kw, int kh, void* stream) {
    if (!x || !y || (C & 7) || kw < 1 || kw > 2 || kh < 1 || kh > 2 || W % kw || H % kh) return OCR_ERR_INVALID;
    long total = (long)Nb * (W / kw) * (H / kh) * (C >> 3);
    const bf16_t* xi = (const bf16_t*)x; bf16_t* yo = (bf16_t*)y;
    hipStream_t st = (hipStream_t)stream;
    int gr = grid_for(total, 8192);
    if (kw == 2 && kh == 2) maxpool_fwd_kernel<2, 2><<<gr, 256, 0, st>>>(xi, yo, Nb, W, H, C);
    else if (kw == 1 && kh == 2) maxpool_fwd_kernel<1, 2><<<gr, 256, 0, st>>>(xi, yo, Nb, W, H, C);
    else if (kw == 2 && kh == 1) maxpool_fwd_kernel<2, 1><<<gr, 256, 0, st>>>(xi, yo, Nb, W, H, C);
    else return OCR_ERR_INVALID;
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_maxpool_bwd(const void* x, const void* dy, void* dx, int Nb, int W, int H, int C, int kw, int kh,
                               int relu_mask, void* stream) {
    if (!x || !dy || !dx || (C & 7) || kw < 1 || kw > 2 || kh < 1 || kh > 2 || W % kw || H % kh) return OCR_ERR_INVALID;
    long total = (long)Nb * (W / kw) * (H / kh) * (C >> 3);
    const bf16_t* xi = (const bf16_t*)x; const bf16_t* dyi = (const bf16_t*)dy; bf16_t* dxo = (bf16_t*)dx;
    hipStream_t st = (hipStream_t)stream;
    int gr = grid_for(total, 8192);
    if (kw == 2 && kh == 2) maxpool_bwd_kernel<2, 2><<<gr, 256, 0, st>>>(xi, dyi, dxo, Nb, W, H, C, relu_mask);
    else if (kw == 1 && kh == 2) maxpool_bwd_kernel<1, 2><<<gr, 256, 0, st>>>(xi, dyi, dxo, Nb, W, H, C, relu_mask);
    else if (kw == 2 && kh == 1) maxpool_bwd_kernel<2, 1><<<gr, 256, 0, st>>>(xi, dyi, dxo, Nb, W, H, C, relu_mask);
    else return OCR_ERR_INVALID;
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
// ocr_maxpool_bwd from the routing codes of the forward pass (uint32 [Nb * W/kw * H/kh][C / 8], 4 bits per channel: index of the first maximum
// in TF scan order | (maximum > 0) << 2) instead of the pool's full-resolution input: bit-identical dx.  Windows (2, 2) and (1, 2).
extern "C" int ocr_maxpool_bwd_codes(const void* codes, const void* dy, void* dx, int Nb, int W, int H, int C, int kw, int kh,
                                     int relu_mask, void* stream) {
    if (!codes || ((size_t)codes & 3) || !dy || !dx || (C & 7) || Nb <= 0 || W <= 0 || H <= 0 || kh != 2 || kw < 1 || kw > 2 || W % kw || H % kh)
        return OCR_ERR_INVALID;
    long total = (long)Nb * (W / kw) * (H / kh) * (C >> 3);
    const uint32_t* ci = (const uint32_t*)codes; const bf16_t* dyi = (const bf16_t*)dy; bf16_t* dxo = (bf16_t*)dx;
    hipStream_t st = (hipStream_t)stream;
    int gr = grid_for(total, 8192);
    if (kw == 2) maxpool_bwd_codes_kernel<2, 2><<<gr, 256, 0, st>>>(ci, dyi, dxo, Nb, W, H, C, relu_mask);
    else maxpool_bwd_codes_kernel<1, 2><<<gr, 256, 0, st>>>(ci, dyi, dxo, Nb, W, H, C, relu_mask);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
// workspace: ocr_bn_workspace_bytes(M, C) bytes = per-block partial rows (fp32) followed by 2*C doubles; not zeroed, no atomics
extern "C" size_t ocr_bn_workspace_bytes(long M, int C) {
    if (M <= 0 || C <= 0) return 0;
    const long nblk = ceil_div(M, (long)bn_rows_per_block_host(M, 512));      // the larger of the two passes' block counts
    return (size_t)nblk * 2 * C * sizeof(float) + 2 * (size_t)C * sizeof(double);
}
// partial_rows > 0: the workspace already holds that many partial rows [rows][2][C] (sum, sum of squares) written by the producing
// convolution (ocr_conv3x3_bf16_stats) — no statistics pass over x.  pooled != NULL: the 1 x 2 max-pool over row pairs that follows the layer
// is written by the apply pass as well (M even, no residual).
// rows per THREAD of the batch-norm apply passes (a thread first loads its 8 channels' 32-40 parameters, then streams rows).  Measured in
// round 4 (profiles/r04n_bn_rows_ab.log): 4 and 8 equal (1.2621-1.2630 / 1.2625-1.2640 ms per step), 16 slower (1.272-1.275: too few blocks).
static constexpr int bn_rows_per_thread() { return 4; }
static int bn_train_fwd_impl(const void* x, void* y, const float* gamma, const float* beta, float* save_mean,
                             float* save_rstd, long M, int C, float eps, int relu, void* workspace, const void* residual,
                             int partial_rows, void* pooled, void* codes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (codes ? (!pooled || ((size_t)codes & 3)) : !y) return OCR_ERR_INVALID;      // the codes form writes no y
    if (!x || !gamma || !beta || !save_mean || !save_rstd || !workspace || (C & 7) || C > 2048 || M <= 0)
        return OCR_ERR_INVALID;
    int rlanes = 256 / (C >> 3); if (rlanes < 1) return OCR_ERR_INVALID;
    if (partial_rows < 0 || (size_t)partial_rows * 2 * C * sizeof(float) > ocr_bn_workspace_bytes(M, C) - 2 * (size_t)C * sizeof(double)) return OCR_ERR_INVALID;
    if (pooled && ((M & 1) || residual)) return OCR_ERR_INVALID;
#ifdef OCR_EXPERIMENTS
    if (!partial_rows && !pooled) {
        int frpb = 0;
        const int fnb = bnf_blocks(M, C, &frpb);
        if (fnb > 0) {
            bn_fused_fwd_kernel<<<fnb, 256, 0, stream>>>((const bf16_t*)x, (bf16_t*)y, gamma, beta, save_mean, save_rstd, (float*)workspace, M, C,
                                                         eps, relu, frpb, (const bf16_t*)residual);
            OCR_CHECK_LAUNCH();
            return OCR_OK;
        }
    }
#endif
    const int rpb = bn_rows_per_block_host(M, 256);
    int nblk = (int)ceil_div(M, (long)rpb);
    if (partial_rows > 0) nblk = partial_rows;
    else {
        bn_stats_kernel<<<nblk, 256, 0, stream>>>((const bf16_t*)x, (float*)workspace, M, C, rpb);
        OCR_CHECK_LAUNCH();
    }
    bn_finalize_kernel<<<ceil_div(C, 16), 256, 0, stream>>>((const float*)workspace, nblk, save_mean, save_rstd, M, C, eps);
    OCR_CHECK_LAUNCH();
    const int arows = bn_rows_per_thread() * rlanes;                // rows per block of the apply pass
    if (pooled)
        bn_apply_pool_kernel<<<ceil_div(M / 2, (long)(arows / 2)), 256, 0, stream>>>((const bf16_t*)x, (bf16_t*)y, (bf16_t*)pooled, save_mean, save_rstd,
                                                                                       gamma, beta, M, C, relu, arows / 2, (uint32_t*)codes);
    else
        bn_apply_kernel<<<ceil_div(M, (long)arows), 256, 0, stream>>>((const bf16_t*)x, (bf16_t*)y, save_mean, save_rstd, gamma,
                                                                        beta, M, C, relu, arows, (const bf16_t*)residual);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_bn_train_fwd(const void* x, void* y, const float* gamma, const float* beta, float* save_mean,
                                float* save_rstd, long M, int C, float eps, int relu, void* workspace, const void* residual, void* stream_) {
    return bn_train_fwd_impl(x, y, gamma, beta, save_mean, save_rstd, M, C, eps, relu, workspace, residual, 0, nullptr, nullptr, stream_);
}
extern "C" int ocr_bn_train_fwd2(const void* x, void* y, const float* gamma, const float* beta, float* save_mean, float* save_rstd, long M,
                                 int C, float eps, int relu, void* workspace, const void* residual, int partial_rows, void* pooled, void* stream_) {
    return bn_train_fwd_impl(x, y, gamma, beta, save_mean, save_rstd, M, C, eps, relu, workspace, residual, partial_rows, pooled, nullptr, stream_);
}
// ocr_bn_train_fwd2 with pooled != NULL whose apply pass writes the pool's routing codes (uint32 [M / 2][C / 8], the format of
// ocr_maxpool_bwd_codes, window 1 x 2) INSTEAD of y (may be NULL): the training form where the pool is the layer's only consumer —
// ocr_bn_train_bwd_codes takes from the codes what the backward passes would read from y.
extern "C" int ocr_bn_train_fwd_codes(const void* x, const float* gamma, const float* beta, float* save_mean, float* save_rstd, long M, int C,
                                      float eps, int relu, void* workspace, int partial_rows, void* pooled, void* codes, void* stream_) {
    if (!codes) return OCR_ERR_INVALID;
    return bn_train_fwd_impl(x, nullptr, gamma, beta, save_mean, save_rstd, M, C, eps, relu, workspace, nullptr, partial_rows, pooled, codes, stream_);
}
// pooled_dy: dy is the gradient of the 1 x 2 max-pool that consumes the layer ([M / 2][C]); both passes route it themselves (first maximum of
// the row pair, bn_pool_route) instead of reading a full-resolution gradient that a max-pool backward pass wrote.
// partial_rows > 0: `dy` is already the ReLU-masked gradient and the workspace holds that many rows [rows][2][C] of (sum dz, sum dz * xhat) written
// by the data-gradient kernel that produced it (ocr_conv3x3_dgrad_bnbwd_bf16): no statistics pass, and the apply pass reads neither y nor a mask.
// cs != NULL (with codes): `dy` is the pooled gradient's buffer, WRITTEN by the statistics pass from the column matrix cs->col (conv5's col2im
// inside it) and read by the apply pass as usual.
struct BnColSrc { const void* col; int Nb, W, HC; };
static int bn_train_bwd_impl(const void* x, const void* y, const void* dy, void* dx, const float* gamma,
                             const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta, long M,
                             int C, int relu, void* workspace, int pooled_dy, int partial_rows, const void* codes, void* stream_,
                             const BnColSrc* cs = nullptr) {
    hipStream_t stream = (hipStream_t)stream_;
    if (cs && (!codes || !cs->col || cs->Nb <= 0 || cs->W <= 0 || cs->HC <= 0 || (cs->HC & 7) || ((size_t)cs->col & 15) || ((size_t)dy & 15) ||
               (long)cs->Nb * cs->W * cs->HC != (M >> 1) * C || (long)cs->Nb * cs->W * (cs->HC >> 3) >= 0x7fffffffL))
        return OCR_ERR_INVALID;
    if (codes ? (!pooled_dy || ((size_t)codes & 3)) : !y) return OCR_ERR_INVALID;      // the codes stand in for y
    if (!x || !dy || !dx || !gamma || !save_mean || !save_rstd || !dgamma || !dbeta || !workspace || (C & 7) ||
        C > 2048 || M <= 0 || (pooled_dy && (M & 1)) || partial_rows < 0 || (partial_rows && pooled_dy))
        return OCR_ERR_INVALID;
    const int rpb = bn_rows_per_block_host(M, 512);
    const int nblk = (int)ceil_div(M, (long)rpb);
    float* part = (float*)workspace;
    double* sums = (double*)((char*)workspace + (size_t)nblk * 2 * C * sizeof(float));
#ifdef OCR_EXPERIMENTS
    {
        int frpb = 0;
        const int fnb = (pooled_dy || partial_rows) ? 0 : bnf_blocks(M, C, &frpb);
        if (fnb > 0) {
            bn_fused_bwd_kernel<<<fnb, 256, 0, stream>>>((const bf16_t*)x, (const bf16_t*)y, (const bf16_t*)dy, (bf16_t*)dx, save_mean, save_rstd,
                                                         gamma, part, sums, dgamma, dbeta, M, C, relu, frpb);
            OCR_CHECK_LAUNCH();
            return OCR_OK;
        }
    }
#endif
    if (partial_rows > nblk) return OCR_ERR_INVALID;                 // the partial rows share the block rows' space in front of `sums`
    if (partial_rows) relu = 0;                                       // premasked
    else {
        if (cs) bn_bwd_stats_col_kernel<<<nblk, 256, 0, stream>>>((const bf16_t*)x, (const bf16_t*)cs->col, cs->W, cs->HC, (bf16_t*)dy, save_mean,
                                                                  save_rstd, part, M, C, rpb, relu, (const uint32_t*)codes);
        else if (codes) bn_bwd_stats_kernel<true><<<nblk, 256, 0, stream>>>((const bf16_t*)x, (const bf16_t*)y, (const bf16_t*)dy, save_mean,
                                                                    save_rstd, part, M, C, rpb, relu, pooled_dy, (const uint32_t*)codes);
        else bn_bwd_stats_kernel<false><<<nblk, 256, 0, stream>>>((const bf16_t*)x, (const bf16_t*)y, (const bf16_t*)dy, save_mean,
                                                                   save_rstd, part, M, C, rpb, relu, pooled_dy, nullptr);
        OCR_CHECK_LAUNCH();
    }
    bn_bwd_finalize_kernel<<<ceil_div(C, 16), 256, 0, stream>>>(part, partial_rows ? partial_rows : nblk, sums, dgamma, dbeta, C);
    OCR_CHECK_LAUNCH();
    const int arows = bn_rows_per_thread() * (256 / (C >> 3));      // rows per block of the apply pass
    if (codes) bn_bwd_apply_kernel<true><<<ceil_div(M, (long)arows), 256, 0, stream>>>((const bf16_t*)x, (const bf16_t*)y, (const bf16_t*)dy,
                                                                                       (bf16_t*)dx, save_mean, save_rstd, gamma, sums, dgamma, dbeta,
                                                                                       M, C, relu, arows, pooled_dy, (const uint32_t*)codes);
    else bn_bwd_apply_kernel<false><<<ceil_div(M, (long)arows), 256, 0, stream>>>((const bf16_t*)x, (const bf16_t*)y, (const bf16_t*)dy,
                                                                                      (bf16_t*)dx, save_mean, save_rstd, gamma, sums, dgamma, dbeta,
                                                                                      M, C, relu, arows, pooled_dy, nullptr);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_bn_train_bwd(const void* x, const void* y, const void* dy, void* dx, const float* gamma,
                                const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta, long M,
                                int C, int relu, void* workspace, void* stream_) {
    return bn_train_bwd_impl(x, y, dy, dx, gamma, save_mean, save_rstd, dgamma, dbeta, M, C, relu, workspace, 0, 0, nullptr, stream_);
}
extern "C" int ocr_bn_train_bwd2(const void* x, const void* y, const void* dy, void* dx, const float* gamma, const float* save_mean,
                                 const float* save_rstd, float* dgamma, float* dbeta, long M, int C, int relu, void* workspace,
                                 int pooled_dy, int partial_rows, void* stream_) {
    return bn_train_bwd_impl(x, y, dy, dx, gamma, save_mean, save_rstd, dgamma, dbeta, M, C, relu, workspace, pooled_dy, partial_rows, nullptr, stream_);
}
// ocr_bn_train_bwd2(pooled_dy = 1) from the codes of ocr_bn_train_fwd_codes instead of y: bit-identical dx, dgamma and dbeta.
extern "C" int ocr_bn_train_bwd_codes(const void* x, const void* codes, const void* dy, void* dx, const float* gamma, const float* save_mean,
                                      const float* save_rstd, float* dgamma, float* dbeta, long M, int C, int relu, void* workspace, void* stream_) {
    if (!codes) return OCR_ERR_INVALID;
    return bn_train_bwd_impl(x, nullptr, dy, dx, gamma, save_mean, save_rstd, dgamma, dbeta, M, C, relu, workspace, 1, 0, codes, stream_);
}
// ocr_conv5_col2im(col, dy_pooled_out, Nb, W, HC) + ocr_bn_train_bwd_codes with the overlap-add inside the statistics pass (one launch and one
// pass over the pooled gradient less): dy_pooled_out, dx, dgamma and dbeta are the same bits.
extern "C" int ocr_bn_train_bwd_codes_col(const void* x, const void* codes, const void* col, int Nb, int W, int HC, void* dy_pooled_out, void* dx,
                                          const float* gamma, const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta, long M,
                                          int C, int relu, void* workspace, void* stream_) {
    if (!codes || !col) return OCR_ERR_INVALID;
    const BnColSrc cs = {col, Nb, W, HC};
    return bn_train_bwd_impl(x, nullptr, dy_pooled_out, dx, gamma, save_mean, save_rstd, dgamma, dbeta, M, C, relu, workspace, 1, 0, codes, stream_, &cs);
}
extern "C" int ocr_colsum_bf16(const void* a, float* out, long M, int C, long lda, void* stream) {
    if (!a || !out || (C & 7) || C > 2048 || M <= 0) return OCR_ERR_INVALID;
    int rpb = 128;
    colsum_kernel<<<ceil_div(M, rpb), 256, 0, (hipStream_t)stream>>>((const bf16_t*)a, out, M, C, lda, rpb);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_pack_transpose(const float* in, void* out, int R, int Cc, long ldin, int lstm_units, void* stream) {
    if (!in || !out || R <= 0 || Cc <= 0) return OCR_ERR_INVALID;
    if (lstm_units > 0 && Cc != 4 * lstm_units) return OCR_ERR_INVALID;
    dim3 grid(ceil_div(Cc, 32), ceil_div(R, 32));
    pack_transpose_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(in, (bf16_t*)out, R, Cc, ldin, lstm_units);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_pack_conv_dgrad(const float* w, void* out, int Cin, int Cout, void* stream) {
    if (!w || !out) return OCR_ERR_INVALID;
    pack_conv_dgrad_kernel<<<grid_for(9L * Cin * Cout), 256, 0, (hipStream_t)stream>>>(w, (bf16_t*)out, Cin, Cout);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
// jobs: device array of `njobs` PackJob records (layout above), block_start ascending, total_blocks = sum of nblocks
extern "C" int ocr_pack_jobs(const void* jobs, int njobs, int total_blocks, void* stream) {
    if (!jobs || njobs <= 0 || total_blocks <= 0) return OCR_ERR_INVALID;
    pack_jobs_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>((const PackJob*)jobs, njobs);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_cast_f32_bf16(const float* in, void* out, long n, void* stream) {
    if (!in || !out || n < 0) return OCR_ERR_INVALID;
    if (n == 0) return OCR_OK;
    cast_f32_bf16_kernel<<<grid_for((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(in, (bf16_t*)out, n);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
// pixels as the generator produces them (uint8) -> the fp32 [0, 1] input the graph is fed with: x = u8 / 255 exactly as
// numpy's `astype(float32) / 255.` does on the host (gen.py:59-65) — IEEE division, not a multiply by 1/255
__global__ void u8_to_unit_f32_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, long n4) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint32_t p = ((const uint32_t*)in)[i];
        f32x4 v = {__fdiv_rn((float)(p & 0xff), 255.0f), __fdiv_rn((float)((p >> 8) & 0xff), 255.0f),
                   __fdiv_rn((float)((p >> 16) & 0xff), 255.0f), __fdiv_rn((float)(p >> 24), 255.0f)};
        ((f32x4*)out)[i] = v;
    }
}
extern "C" int ocr_u8_to_unit_f32(const void* in, float* out, long n, void* stream) {
    if (!in || !out || n < 0 || (n & 3)) return OCR_ERR_INVALID;
    if (n == 0) return OCR_OK;
    u8_to_unit_f32_kernel<<<grid_for(n / 4), 256, 0, (hipStream_t)stream>>>((const uint8_t*)in, out, n / 4);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
// One launch that makes a device-resident batch the graph's input: pixels (uint8 -> x / 255, or fp32 copied) plus the three
// small int32 vectors.  Four separate D2D copies were four blit kernels (~5 us each) with a queue barrier in front of each.
__global__ void bind_batch_kernel(const void* __restrict__ pix, int is_u8, float* __restrict__ x, long n4,
                                  const int* __restrict__ s0, int* __restrict__ d0, int n0, const int* __restrict__ s1, int* __restrict__ d1, int n1,
                                  const int* __restrict__ s2, int* __restrict__ d2, int n2) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        if (is_u8) {
            const uint32_t p = ((const uint32_t*)pix)[i];
            ((f32x4*)x)[i] = (f32x4){__fdiv_rn((float)(p & 0xff), 255.0f), __fdiv_rn((float)((p >> 8) & 0xff), 255.0f),
                                     __fdiv_rn((float)((p >> 16) & 0xff), 255.0f), __fdiv_rn((float)(p >> 24), 255.0f)};
        } else {
            ((f32x4*)x)[i] = ((const f32x4*)pix)[i];
        }
    }
    if (blockIdx.x == gridDim.x - 1) {
        for (int i = threadIdx.x; i < n0; i += blockDim.x) d0[i] = s0[i];
        for (int i = threadIdx.x; i < n1; i += blockDim.x) d1[i] = s1[i];
        for (int i = threadIdx.x; i < n2; i += blockDim.x) d2[i] = s2[i];
    }
}
extern "C" int ocr_bind_batch(const void* pixels, int pixels_are_u8, float* x, long n_pixels, const int* seq_len, int* seq_len_dst, int n_seq,
                              const int* labels, int* labels_dst, int n_labels, const int* labels_len, int* labels_len_dst, int n_labels_len,
                              void* stream) {
    if (!pixels || !x || n_pixels <= 0 || (n_pixels & 3) || n_seq < 0 || n_labels < 0 || n_labels_len < 0) return OCR_ERR_INVALID;
    if ((n_seq && (!seq_len || !seq_len_dst)) || (n_labels && (!labels || !labels_dst)) || (n_labels_len && (!labels_len || !labels_len_dst)))
        return OCR_ERR_INVALID;
    if (((size_t)pixels & (pixels_are_u8 ? 3 : 15)) || ((size_t)x & 15)) return OCR_ERR_INVALID;
    bind_batch_kernel<<<grid_for(n_pixels / 4), 256, 0, (hipStream_t)stream>>>(pixels, pixels_are_u8, x, n_pixels / 4, seq_len, seq_len_dst, n_seq,
                                                                              labels, labels_dst, n_labels, labels_len, labels_len_dst, n_labels_len);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
// Everything the training loop reads back after a step, gathered into 4 doubles so that ONE 32-byte D2H copy follows:
// out[0] = mean per-sample CTC cost (summed in double, fixed order), out[1] = scalars[1] (sum w^2 of the regularised range),
// out[2] = scalars[7] (global gradient norm), out[3] = bit i set <=> error word i (last int of words[i]) is 1 (the persistent LSTM kernels' time-out mark),
// bit 40 set <=> the update of this step was dropped on the device (scalars[72]).
__global__ void step_report_kernel(const float* __restrict__ costs, int n, const double* __restrict__ scalars,
                                   const long long* __restrict__ words, int nwords, double* __restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) s += (double)costs[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) {
        unsigned bits = 0;
        for (int i = 0; i < nwords; ++i) if (*(const int*)words[i] == 1) bits |= 1u << i;    // 0 or, in a caller-prepared block, all ones: no time-out
        out[0] = s / (double)n;
        out[1] = scalars ? scalars[1] : 0.0;
        out[2] = scalars ? scalars[7] : 0.0;
        // + 2^40 when THIS step's update was dropped by the guarded optimiser step (scalars[72]: the report is queued right behind the step, so the
        // word is the step's own — the host decides per step instead of comparing a global counter: ADVICE r5)
        out[3] = (double)bits + ((scalars && scalars[72] != 0.0) ? 1099511627776.0 : 0.0);
    }
}
extern "C" int ocr_step_report(const float* costs, int n, const double* scalars, const void* word_addrs, int nwords, double* out, void* stream) {
    if (!costs || n <= 0 || !out || nwords < 0 || nwords > 32 || (nwords && !word_addrs)) return OCR_ERR_INVALID;
    step_report_kernel<<<1, 64, 0, (hipStream_t)stream>>>(costs, n, scalars, (const long long*)word_addrs, nwords, out);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_cast2d_f32_bf16(const float* in, long ldin, void* out, long ldout, int rows, int cols, void* stream) {
    if (!in || !out || rows <= 0 || cols <= 0 || (cols & 3) || (ldin & 3) || (ldout & 3)) return OCR_ERR_INVALID;
    cast2d_f32_bf16_kernel<<<grid_for((long)rows * (cols >> 2)), 256, 0, (hipStream_t)stream>>>(in, ldin, (bf16_t*)out, ldout, rows, cols);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_tnc_to_ntc_bf16(const float* in, void* out, int T, int N, int C, float scale, void* stream) {
    if (!in || !out) return OCR_ERR_INVALID;
    tnc_to_ntc_bf16_kernel<<<grid_for((long)T * N * C), 256, 0, (hipStream_t)stream>>>(in, (bf16_t*)out, T, N, C, scale);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
extern "C" int ocr_conv5_col2im(const void* col, void* dx, int Nb, int W, int HC, void* stream) {
    if (!col || !dx) return OCR_ERR_INVALID;
    if (!col2im_v1() && (HC & 7) == 0 && (long)Nb * W * (HC >> 3) < 0x7fffffffL && ((size_t)col & 15) == 0 && ((size_t)dx & 15) == 0)
        conv5_col2im8_kernel<<<grid_for((long)Nb * W * (HC >> 3), 2048), 256, 0, (hipStream_t)stream>>>((const bf16_t*)col, (bf16_t*)dx, Nb, W, HC);
    else
        conv5_col2im_kernel<<<grid_for((long)Nb * W * HC), 256, 0, (hipStream_t)stream>>>((const bf16_t*)col, (bf16_t*)dx, Nb, W, HC);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
