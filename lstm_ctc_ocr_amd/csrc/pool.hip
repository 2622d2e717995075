#include "common.h"

// ============================================================================================
// max-pool (VALID, window == stride, kw over axis W in {1,2}, kh over axis H in {1,2})
//   reference: Network.max_pool  network.py:343-350 ; LSTM_train.py:25,27,30,33
// ============================================================================================
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
