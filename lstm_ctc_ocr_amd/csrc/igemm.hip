// Large-tile bf16 MFMA engine for gfx950 (second generation of gemm.hip's kernel, same contract):
//     out[m][n] = sum_k P[m][k] * Q[n][k]      P = activations / pixels, Q = weights, both K-contiguous
// used for the 3x3 SAME implicit-GEMM convolutions (forward and data gradient — reference
// lib/networks/network.py:160-191 via tf.nn.conv2d) and for the large plain GEMMs.
//
// What changed against gemm.hip and why (measured there: 370-570 TFLOP/s, every pipe ~equally loaded —
// MFMA 256, LDS 340, L1 fill 256, TA 256 cycles per 128x128x32 step — so nothing overlapped well):
//   * block tile 256 (m) x BN (n in {64,128,256}), BK = 64, 8 waves (512 threads): operand bytes per flop halve,
//     MFMA becomes the longest pipe (1024 cyc/SIMD/step vs 512 LDS-read, 768 L1-fill at BN = 128);
//   * global -> LDS by LDS-DMA (`global_load_lds_dwordx4`, 1 KiB per wave instruction = 8 rows x 128 B): no staging
//     VGPRs, no ds_write pass; two LDS stages, the next K tile streams in while the current one feeds the MFMAs;
//   * the LDS image is row-linear (DMA writes lane-linearly), so the XOR swizzle that makes the 16-row ds_read_b128
//     fragment reads conflict-free is applied to the SOURCE chunk (chunk ^ (row & 7)) and again on the read;
//   * SAME-padding halo and M/N tails read from a 64-B zero page instead of branching (DMA cannot skip a lane);
//   * workgroup ids are remapped so each XCD (private 4 MiB L2) owns a contiguous range of tiles: the 9 taps and
//     the neighbouring m-tiles re-read the same activation rows out of that XCD's L2.
// MFMA orientation and epilogue are unchanged: A := Q tile, B := P tile, each lane owns 4 consecutive n of one m.
// The workgroup itself is igemm_body.h's ig_body (gemm_tn3.hip's paired launch runs it too).
#include "igemm_body.h"
#include <stdlib.h>

__device__ u32x4 ig_zero_page[4];   // 64 B of zeros (device globals are zero-initialised)

template <int BN, int MODE, int STAGES, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2, 2))) void igemm_kernel(IgArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ig_body<BN, MODE, STAGES, NW>(g, (int)blockIdx.x, smem, (const bf16_t*)ig_zero_page);
}

int g_ig_stages = 3;     // A/B knob (ocr_set_gemm_engine): 3 = three-stage counted-vmcnt pipeline where LDS allows, 2 = two-stage

template <int BN, int MODE, int STAGES, int NW>
static int launch_ig2(const IgArgs& g, hipStream_t stream) {
    constexpr int BM = 32 * NW;
    constexpr int LDS = ig_lds_bytes<BN, STAGES, NW>();
    if (ocr_allow_lds<igemm_kernel<BN, MODE, STAGES, NW>>(LDS) != hipSuccess) return OCR_ERR_EXEC;
    int mt = (g.M + BM - 1) / BM, nt = (g.N + BN - 1) / BN;
    igemm_kernel<BN, MODE, STAGES, NW><<<mt * nt, 64 * NW, LDS, stream>>>(g);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
template <int BN, int MODE>
static int launch_ig(const IgArgs& g, hipStream_t stream) {
    if (BN <= 128 && g_ig_stages == 3) return launch_ig2<(BN <= 128 ? BN : 128), MODE, 3, 8>(g, stream);   // 3 x 48 KiB fits, 3 x 64 KiB does not
    return launch_ig2<BN, MODE, 2, 8>(g, stream);
}

// Shared with gemm.hip's entry points: returns -1 when the shape is not covered (caller uses the small-tile kernel).
int ig_try_dispatch(const void* P, long ldp, const void* Q, long ldq, void* out, long ldo, int M, int N, int K,
                    const float* bias, const void* mask, long ldmask, int flags, int mode, int grp, int skip, int cW,
                    int cH, int cC, int swap_inner, int swap_outer, hipStream_t stream) {
    if (!ig_covers(M, N, K, flags, mode, cC)) return -1;
    IgArgs g = {};
    g.P = (const bf16_t*)P; g.Q = (const bf16_t*)Q; g.ldp = ldp; g.ldq = ldq; g.M = M; g.N = N; g.K = K;
    g.grp = grp; g.skip = skip; g.cW = cW; g.cH = cH; g.cC = cC; g.out = out; g.ldo = ldo; g.bias = bias;
    g.mask = (const bf16_t*)mask; g.ldmask = ldmask; g.flags = flags; g.swap_inner = swap_inner; g.swap_outer = swap_outer;
    // 128-row tiles of 4 waves (72 KiB of LDS with three stages at BN = 64, 64 KiB with two at BN = 128: two workgroups per
    // CU) when the 256-row grid cannot give every CU two waves' worth of work — the M = 4032 GEMMs of conv5 / LSTM / FC.
    static int ig_nw = -1;                                 // A/B knob OCR_IG_NW: 8 / 4 force, unset = by grid size
    if (ig_nw < 0) { const char* e = ocr_tune_env("OCR_IG_NW"); ig_nw = e ? atoi(e) : 0; }
    if (mode == 0 && ig_nw != 8) {
        const long mt4 = (M + 127) / 128;
        const long wg8 = (long)((M + 255) / 256) * ((N + 127) / 128);
        if (ig_nw == 4 || wg8 < 400) {
            if (N >= 128 && mt4 * ((N + 127) / 128) >= 448) return launch_ig2<128, 0, 2, 4>(g, stream);
            return launch_ig2<64, 0, 3, 4>(g, stream);
        }
    }
    const int mt = (M + 255) / 256;
    int bn = 64;                                           // widest n-tile that still gives every CU a workgroup
    if (N >= 256 && (long)mt * ((N + 255) / 256) >= 256) bn = 256;
    else if (N >= 128 && (long)mt * ((N + 127) / 128) >= 256) bn = 128;
    else if (N >= 128 && (long)mt * ((N + 63) / 64) < 96) bn = 128;    // tiny grid either way: fewer, fatter tiles
#define IG_CASE(BNV)                                                                  \
    if (bn == BNV) return mode == 1 ? launch_ig<BNV, 1>(g, stream) : launch_ig<BNV, 0>(g, stream);
    IG_CASE(256) IG_CASE(128) IG_CASE(64)
#undef IG_CASE
    return -1;
}
