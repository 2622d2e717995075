// The first layer for gfx950: conv1 (C_in = 1, K = 9: VALU, not MFMA) at full resolution, its weight gradient, and
// the fused conv1 + ReLU + 2x2 max-pool forward and backward on a staged LDS tile.  Every kernel stands next to the entry point that launches
// it; everything moves 16 B per lane (8 bf16 / 4 f32), coalesced along the channel axis of the reference layout [N, W, H, C].
#include "common.h"
#include <stdlib.h>
#include <algorithm>

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
extern "C" int ocr_conv1_wgrad(const float* x, const void* dz, float* dw, float* db, int Nb, int W, int H, int Cout,
                               void* stream) {
    if (!x || !dz || !dw || !db || Cout != 64) return OCR_ERR_INVALID;
    long npix = (long)Nb * W * H;
    int ppb = 1024;
    conv1_wgrad_kernel<<<ceil_div(npix, ppb), 256, 0, (hipStream_t)stream>>>(x, (const bf16_t*)dz, dw, db, Nb, W, H, Cout, ppb);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
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
// at +0 never becomes -0, so neither does accumulator + bias), hence pool_code2_u16's integer order is the float order: the code of a channel is
// the index of the FIRST maximum of the window's four bf16-ROUNDED outputs in scan order e = 2 (w offset) + (h offset) | (that maximum > 0) << 2
// — what a max-pool backward on the stored tensor would decide (common.h: pool_code_word) — and max-then-round == round-then-max.
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
    const Conv1Launch L = conv1_launch(Nb, W, H, conv1_fwd_ppb());
    if (!L.ok) return OCR_ERR_INVALID;
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
// The routing word of a pixel's channel group holds 4 bits per channel: bits 0-1 = window element `best` (first maximum of the bf16-rounded
// outputs, e = 2 (w offset) + (h offset)), bit 2 = (maximum > 0); saved by the forward pass (CODES) or recomputed here with its arithmetic.
// Routing without a lookup: the gradient of a pooled output goes to window element `best`, i.e. tap t multiplies
// patch[(best >> 1) + t / 3][(best & 1) + t % 3].  Instead of addressing the patch per channel, g_e = (best == e) ? gv : 0 for the four elements
// and ALL 4 x 9 fused multiply-adds are issued per channel pair on the register-held patch: fma(p, 0, acc) == acc for finite p (acc is never
// -0), so each accumulator sees exactly one effective fma per pixel, in pixel order — 144 v_pk_fma_f32 and no LDS traffic beyond the 16
// broadcast reads of the patch.  (Reading the taps straight from the shared tile at data-dependent offsets — 72 LDS reads + 36 v_pk_fma_f32 —
// measured 19.0 us against 17.3 at 64 x 256 x 32 and 24.9 against 22.1 at 64 x 320 x 32, profiles/r12_conv1_kernels.log.)
template <bool CODES /* routing + ReLU bits from the forward pass: no window recomputation */>
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
    float acc[10][8];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) { acc[t][2 * q] = acc2[t][q].x; acc[t][2 * q + 1] = acc2[t][q].y; }
    conv1_bwd_reduce(acc, dw, db, slab);
}
// pooled pixels per block of the conv1 + pool backward kernel (a thread walks ppb / 32 of them, one memory round trip each).  With atomics
// smaller blocks were slower (profiles/r04k_conv1_ppb_ab.log: 640 same-address atomics per block); the slab form pays 2.5 KB per block instead.
static int conv1_ppb() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("OCR_CONV1_PPB"); v = e ? atoi(e) : 256; if (v < 32 || v > 1024 || (v & 31)) v = 256; }
    return v;
}
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
    if (codes) {
        if (ocr_allow_lds<conv1_pool_bwd_tile_kernel<true>>(L.lds) != hipSuccess) return OCR_ERR_EXEC;
        conv1_pool_bwd_tile_kernel<true><<<nb, 256, L.lds, (hipStream_t)stream>>>(x, w, bias, g, dw, db, Nb, W, H, ppb, L.rH, L.rHo, L.rWo, cd, slab);
    } else {
        if (ocr_allow_lds<conv1_pool_bwd_tile_kernel<false>>(L.lds) != hipSuccess) return OCR_ERR_EXEC;
        conv1_pool_bwd_tile_kernel<false><<<nb, 256, L.lds, (hipStream_t)stream>>>(x, w, bias, g, dw, db, Nb, W, H, ppb, L.rH, L.rHo, L.rWo, nullptr, slab);
    }
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
