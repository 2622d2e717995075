#include "common.h"

// ============================================================================================
// training-mode batch norm over rows of x[M][C] (bf16), biased variance, eps (TF contrib default 1e-3)
//   reference: tf.contrib.layers.batch_norm(..., is_training=True)  network.py:176-178  (always batch stats)
// ============================================================================================
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
