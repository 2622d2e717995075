// Streaming launches of the train step for gfx950 that belong to no layer family: bias-gradient column sums, weight (re)packing and casts,
// the CTC gradient hand-off, conv5's col2im, element-wise ops of residual graphs, input binding and the step report.  Every kernel stands next
// to the entry point that launches it.
#include "common.h"
#include <stdlib.h>

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
extern "C" int ocr_colsum_bf16(const void* a, float* out, long M, int C, long lda, void* stream) {
    if (!a || !out || (C & 7) || C > 2048 || M <= 0) return OCR_ERR_INVALID;
    int rpb = 128;
    colsum_kernel<<<ceil_div(M, rpb), 256, 0, (hipStream_t)stream>>>((const bf16_t*)a, out, M, C, lda, rpb);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
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
extern "C" int ocr_pack_transpose(const float* in, void* out, int R, int Cc, long ldin, int lstm_units, void* stream) {
    if (!in || !out || R <= 0 || Cc <= 0) return OCR_ERR_INVALID;
    if (lstm_units > 0 && Cc != 4 * lstm_units) return OCR_ERR_INVALID;
    dim3 grid(ceil_div(Cc, 32), ceil_div(R, 32));
    pack_transpose_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(in, (bf16_t*)out, R, Cc, ldin, lstm_units);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
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
extern "C" int ocr_pack_conv_dgrad(const float* w, void* out, int Cin, int Cout, void* stream) {
    if (!w || !out) return OCR_ERR_INVALID;
    pack_conv_dgrad_kernel<<<grid_for(9L * Cin * Cout), 256, 0, (hipStream_t)stream>>>(w, (bf16_t*)out, Cin, Cout);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
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
extern "C" int ocr_cast_f32_bf16(const float* in, void* out, long n, void* stream) {
    if (!in || !out || n < 0) return OCR_ERR_INVALID;
    if (n == 0) return OCR_OK;
    cast_f32_bf16_kernel<<<grid_for((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(in, (bf16_t*)out, n);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
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
extern "C" int ocr_cast2d_f32_bf16(const float* in, long ldin, void* out, long ldout, int rows, int cols, void* stream) {
    if (!in || !out || rows <= 0 || cols <= 0 || (cols & 3) || (ldin & 3) || (ldout & 3)) return OCR_ERR_INVALID;
    cast2d_f32_bf16_kernel<<<grid_for((long)rows * (cols >> 2)), 256, 0, (hipStream_t)stream>>>(in, ldin, (bf16_t*)out, ldout, rows, cols);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
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
extern "C" int ocr_tnc_to_ntc_bf16(const float* in, void* out, int T, int N, int C, float scale, void* stream) {
    if (!in || !out) return OCR_ERR_INVALID;
    tnc_to_ntc_bf16_kernel<<<grid_for((long)T * N * C), 256, 0, (hipStream_t)stream>>>(in, (bf16_t*)out, T, N, C, scale);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
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
// OCR_COL2IM_V1=1 (experiments flavour; the product library never reads it: ocr_tune_env): the scalar col2im everywhere (13.3 us against 5.9 for
// the 16-byte one).  The scalar kernel is also the fallback for HC % 8 != 0 / unaligned buffers, which is how the tests reach it.
static bool col2im_v1() {
    static int v = -1;
    if (v < 0) { const char* e = ocr_tune_env("OCR_COL2IM_V1"); v = (e && atoi(e) != 0) ? 1 : 0; }
    return v == 1;
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
// jobs: device array of `njobs` PackJob records (layout above), block_start ascending, total_blocks = sum of nblocks
extern "C" int ocr_pack_jobs(const void* jobs, int njobs, int total_blocks, void* stream) {
    if (!jobs || njobs <= 0 || total_blocks <= 0) return OCR_ERR_INVALID;
    pack_jobs_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>((const PackJob*)jobs, njobs);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
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
extern "C" int ocr_eltwise_bf16(int op, const void* a, const void* b, void* out, long n, void* stream) {
    if (!a || !out || (op != 1 && !b) || op < 0 || op > 4 || n <= 0 || (n & 7)) return OCR_ERR_INVALID;
    eltwise_bf16_kernel<<<grid_for(n / 8, 4096), 256, 0, (hipStream_t)stream>>>(op, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out, n / 8);
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
