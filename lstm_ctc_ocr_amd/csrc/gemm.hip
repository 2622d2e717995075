// bf16 MFMA tile engine for gfx950: C[m][n] = sum_k P[m][k] * Q[n][k]  (both operands K-contiguous)
//
// One engine serves every dense contraction on the CRNN hot path:
//   * a2  conv_single 3x3 SAME  fwd / dgrad as an IMPLICIT GEMM: P rows are output pixels of the
//         reference layout [N, W, H, C] (lib/networks/network.py:160-191), k = (tap, ci); the
//         loader shifts the pixel by the tap and zero-fills the SAME-padding halo.
//   * a2  conv5 2x2 VALID as a plain GEMM over overlapping rows (row-group skip, see below).
//   * a6  the hoisted LSTM input projection, the FC logits (network.py:118-128) and their
//         data-gradient GEMMs.
//
// MFMA orientation: v_mfma_f32_16x16x32_bf16 with A := Q tile (rows -> output channel n) and
// B := P tile (cols -> output row m).  Each lane then owns 4 CONSECUTIVE n of one m, i.e. one
// 8-byte bf16x4 (or 16-byte f32x4) store into the n-contiguous output — no LDS transpose in
// the epilogue.
//
// Tile: 256 threads = 4 waves as 2(m) x 2(n); block tile (32*FM) x (32*FN), BK = 32 per step,
// LDS rows padded to 80 B (5 x 16-B slots: gcd(5,16)=1 spreads a 16-row fragment read over all
// 16 slots of the 256-B bank row).  Global -> register -> LDS staging, next tile's loads issued
// before the current tile's MFMAs (T14-style split).
#include "conv_plan.h"
#include <string.h>

enum {
    EPI_BIAS = 1,        // + bias[n]
    EPI_RELU = 2,        // max(0, .)
    EPI_OUT_F32 = 4,     // fp32 output (else bf16)
    EPI_ATOMIC = 8,      // atomicAdd into fp32 output (split-K)
    EPI_MASK = 16,       // zero where mask[m][n] <= 0 (ReLU backward fused into dgrad)
    EPI_ROWSWAP = 32,    // out row = (m % inner) * outer + m / inner   ([N,T] -> [T,N])
    EPI_ACCUM = 64,      // out += value (fp32, non-atomic; single split only)
};

struct GemmArgs {
    const bf16_t* P;   // m rows
    const bf16_t* Q;   // n rows
    long ldp, ldq;
    int M, N, K;       // K % 8 == 0
    int k_per_split;   // multiple of 32; gridDim.z splits
    // plain-mode row groups: physical row = m + (m / grp) * skip   (conv5's overlapping windows)
    int grp, skip;
    // conv-mode geometry (P = activations [Nb, cW, cH, cC], K = 9*cC, cC % 32 == 0)
    int cW, cH, cC;
    // epilogue
    void* out;
    long ldo;
    const float* bias;
    const bf16_t* mask;
    long ldmask;
    int flags;
    int swap_inner, swap_outer;
};

#define LDS_ROW 40   // bf16 elements per LDS row: 32 payload + 8 pad  (80 B)

template <int MODE /*0 plain, 1 conv3x3*/, int FM, int FN>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs g) {
    constexpr int BM = 32 * FM, BN = 32 * FN;
    constexpr int NCP = BM * 4 / 256;   // 16-B chunks per thread for the P tile
    constexpr int NCQ = BN * 4 / 256;
    __shared__ __attribute__((aligned(16))) bf16_t Ps[BM * LDS_ROW];
    __shared__ __attribute__((aligned(16))) bf16_t Qs[BN * LDS_ROW];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int kbeg = blockIdx.z * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);

    // ---- per-thread staging coordinates (fixed for the whole K loop)
    const bf16_t* prow[NCP];
    bool pvalid[NCP];
    int pw[NCP], ph[NCP];
#pragma unroll
    for (int i = 0; i < NCP; ++i) {
        int c = tid + i * 256;
        int r = c >> 2;
        int m = m0 + r;
        pvalid[i] = m < g.M;
        int mm = pvalid[i] ? m : 0;
        if (MODE == 0) {
            long phys = (long)mm + (g.grp > 0 ? (long)(mm / g.grp) * g.skip : 0);
            prow[i] = g.P + phys * g.ldp + (c & 3) * 8;
            pw[i] = ph[i] = 0;
        } else {
            int h = mm % g.cH;
            int q = mm / g.cH;
            int w = q % g.cW;
            pw[i] = w; ph[i] = h;
            prow[i] = g.P + (long)mm * g.cC + (c & 3) * 8;   // pixel (n,w,h), channel chunk
        }
    }
    const bf16_t* qrow[NCQ];
    bool qvalid[NCQ];
#pragma unroll
    for (int i = 0; i < NCQ; ++i) {
        int c = tid + i * 256;
        int r = c >> 2;
        int n = n0 + r;
        qvalid[i] = n < g.N;
        qrow[i] = g.Q + (long)(qvalid[i] ? n : 0) * g.ldq + (c & 3) * 8;
    }

    u32x4 pst[NCP], qst[NCQ];
    auto load_tiles = [&](int k0) {
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < NCP; ++i) {
                int kc = k0 + ((tid + i * 256) & 3) * 8;
                u32x4 v = {0, 0, 0, 0};
                if (pvalid[i] && kc < kend) v = *(const u32x4*)(prow[i] + k0);
                pst[i] = v;
            }
        } else {
            int tap = k0 / g.cC;            // uniform: cC % 32 == 0 keeps a K tile inside one tap
            int ci0 = k0 - tap * g.cC;
            int dw = tap / 3 - 1, dh = tap % 3 - 1;
            long shift = ((long)dw * g.cH + dh) * g.cC + ci0;
#pragma unroll
            for (int i = 0; i < NCP; ++i) {
                int ww = pw[i] + dw, hh = ph[i] + dh;
                bool ok = pvalid[i] && (unsigned)ww < (unsigned)g.cW && (unsigned)hh < (unsigned)g.cH;
                u32x4 v = {0, 0, 0, 0};
                if (ok) v = *(const u32x4*)(prow[i] + shift);
                pst[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < NCQ; ++i) {
            int kc = k0 + ((tid + i * 256) & 3) * 8;
            u32x4 v = {0, 0, 0, 0};
            if (qvalid[i] && kc < kend) v = *(const u32x4*)(qrow[i] + k0);
            qst[i] = v;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < NCP; ++i) {
            int c = tid + i * 256;
            *(u32x4*)(&Ps[(c >> 2) * LDS_ROW + (c & 3) * 8]) = pst[i];
        }
#pragma unroll
        for (int i = 0; i < NCQ; ++i) {
            int c = tid + i * 256;
            *(u32x4*)(&Qs[(c >> 2) * LDS_ROW + (c & 3) * 8]) = qst[i];
        }
    };

    f32x4 acc[FN][FM];
#pragma unroll
    for (int a = 0; a < FN; ++a)
#pragma unroll
        for (int b = 0; b < FM; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fk = (lane >> 4) * 8;
    if (kbeg < kend) {
        load_tiles(kbeg);
        for (int k0 = kbeg; k0 < kend; k0 += 32) {
            __syncthreads();            // previous tile's fragment reads are done
            store_tiles();
            __syncthreads();
            if (k0 + 32 < kend) load_tiles(k0 + 32);   // in flight during the MFMAs below
            bf16x8 af[FN], bfr[FM];
#pragma unroll
            for (int a = 0; a < FN; ++a)
                af[a] = *(const bf16x8*)(&Qs[(wn * 16 * FN + a * 16 + frow) * LDS_ROW + fk]);
#pragma unroll
            for (int b = 0; b < FM; ++b)
                bfr[b] = *(const bf16x8*)(&Ps[(wm * 16 * FM + b * 16 + frow) * LDS_ROW + fk]);
#pragma unroll
            for (int a = 0; a < FN; ++a)
#pragma unroll
                for (int b = 0; b < FM; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
        }
    }

    // ---- epilogue: lane owns n = nb + (lane>>4)*4 .. +3 at m = mb + (lane&15)
    const int flags = g.flags;
    const bool add_bias = (flags & EPI_BIAS) && (!(flags & EPI_ATOMIC) || blockIdx.z == 0);
#pragma unroll
    for (int a = 0; a < FN; ++a) {
        int n = n0 + wn * 16 * FN + a * 16 + (lane >> 4) * 4;
        if (n >= g.N) continue;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (add_bias) bv = *(const f32x4*)(g.bias + n);
#pragma unroll
        for (int b = 0; b < FM; ++b) {
            int m = m0 + wm * 16 * FM + b * 16 + (lane & 15);
            if (m >= g.M) continue;
            f32x4 v = acc[a][b] + bv;
            if (flags & EPI_RELU) {
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
            if (flags & EPI_MASK) {
                u32x2 mk = *(const u32x2*)(g.mask + (long)m * g.ldmask + n);
                if (!(bf_lo(mk.x) > 0.f)) v.x = 0.f;
                if (!(bf_hi(mk.x) > 0.f)) v.y = 0.f;
                if (!(bf_lo(mk.y) > 0.f)) v.z = 0.f;
                if (!(bf_hi(mk.y) > 0.f)) v.w = 0.f;
            }
            long orow = m;
            if (flags & EPI_ROWSWAP) orow = (long)(m % g.swap_inner) * g.swap_outer + m / g.swap_inner;
            if (flags & EPI_OUT_F32) {
                float* o = (float*)g.out + orow * g.ldo + n;
                if (flags & EPI_ATOMIC) {
                    atomicAdd(o + 0, v.x); atomicAdd(o + 1, v.y); atomicAdd(o + 2, v.z); atomicAdd(o + 3, v.w);
                } else if (flags & EPI_ACCUM) {
                    f32x4 old = *(f32x4*)o;
                    *(f32x4*)o = old + v;
                } else {
                    *(f32x4*)o = v;
                }
            } else {
                u32x2 pk;
                pk.x = pack_bf2(v.x, v.y);
                pk.y = pack_bf2(v.z, v.w);
                *(u32x2*)((bf16_t*)g.out + orow * g.ldo + n) = pk;
            }
        }
    }
}

template <int MODE, int FM, int FN>
static int launch_gemm(const GemmArgs& g, hipStream_t stream) {
    constexpr int BM = 32 * FM, BN = 32 * FN;
    int splits = ceil_div(g.K, g.k_per_split);
    dim3 grid(ceil_div(g.M, BM), ceil_div(g.N, BN), splits);
    gemm_nt_kernel<MODE, FM, FN><<<grid, 256, 0, stream>>>(g);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}

static int dispatch_gemm(GemmArgs& g, int mode, int splits, hipStream_t stream) {
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || (g.K & 7) || (g.N & 3)) return OCR_ERR_INVALID;
    if (!g.P || !g.Q || !g.out) return OCR_ERR_INVALID;
    if (splits < 1) splits = 1;
    int kps = ceil_div(ceil_div(g.K, splits), 32) * 32;
    g.k_per_split = kps;
    if (splits > 1) {   // a split request always means "accumulate into the fp32 output with atomics"
        if (!(g.flags & EPI_OUT_F32) || (g.flags & (EPI_RELU | EPI_MASK | EPI_ACCUM))) return OCR_ERR_INVALID;
        g.flags |= EPI_ATOMIC;
    }
    // big tiles when they still fill the chip, small tiles otherwise
    long big_blocks = (long)ceil_div(g.M, 128) * ceil_div(g.N, 128) * ceil_div(g.K, kps);
    bool big = big_blocks >= 192 && g.N >= 128;
    if (mode == 1) {
        if (g.cC % 32 || g.K != 9 * g.cC) return OCR_ERR_INVALID;
        return big ? launch_gemm<1, 4, 4>(g, stream) : launch_gemm<1, 2, 2>(g, stream);
    }
    return big ? launch_gemm<0, 4, 4>(g, stream) : launch_gemm<0, 2, 2>(g, stream);
}

// large-tile LDS-DMA engine (igemm.hip); returns -1 when it does not cover the shape
int ig_try_dispatch(const void* P, long ldp, const void* Q, long ldq, void* out, long ldo, int M, int N, int K,
                    const float* bias, const void* mask, long ldmask, int flags, int mode, int grp, int skip, int cW,
                    int cH, int cC, int swap_inner, int swap_outer, hipStream_t stream);
static int g_use_igemm = 1, g_use_halo = 1;
extern int g_ig_stages;
// A/B knob. 0 = 128x128 register-staged tiles only; 1 (default) = the tap-reuse convolution kernels (conv3x3_plan) for 3x3 convs +
// LDS-DMA 256-row tiles (three-stage) for plain GEMMs; 2 = LDS-DMA tiles two-stage, no tap-reuse kernels; 3 = LDS-DMA tiles three-stage, none
extern "C" int ocr_set_gemm_engine(int mode) {
    if (mode < 0 || mode > 3) return OCR_ERR_INVALID;
    g_use_igemm = mode != 0; g_use_halo = mode == 1; g_ig_stages = (mode == 2) ? 2 : 3;
    return OCR_OK;
}
bool gemm_uses_igemm() { return g_use_igemm != 0; }   // gemm_tn3.hip's paired launch runs the large-tile engine's workgroups: only while it is on

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" int ocr_gemm_nt_bf16(const void* P, long ldp, const void* Q, long ldq, void* out, long ldo,
                                int M, int N, int K, const float* bias, const void* mask, long ldmask,
                                int flags, int splits, int row_group, int row_skip, int swap_inner,
                                int swap_outer, void* stream) {
    GemmArgs g = {};
    g.P = (const bf16_t*)P; g.Q = (const bf16_t*)Q; g.ldp = ldp; g.ldq = ldq;
    g.M = M; g.N = N; g.K = K; g.grp = row_group; g.skip = row_skip;
    g.out = out; g.ldo = ldo; g.bias = bias; g.mask = (const bf16_t*)mask; g.ldmask = ldmask;
    g.flags = flags & ~EPI_ATOMIC; g.swap_inner = swap_inner; g.swap_outer = swap_outer;
    if ((flags & EPI_BIAS) && !bias) return OCR_ERR_INVALID;
    if ((flags & EPI_MASK) && !mask) return OCR_ERR_INVALID;
    if ((flags & EPI_ROWSWAP) && (swap_inner <= 0 || swap_outer <= 0)) return OCR_ERR_INVALID;
    if (g_use_igemm && splits <= 1 && P && Q && out && M > 0 && N > 0 && K > 0) {
        int rc = ig_try_dispatch(P, ldp, Q, ldq, out, ldo, M, N, K, bias, mask, ldmask, g.flags, 0, row_group, row_skip, 0, 0, 0,
                                 swap_inner, swap_outer, (hipStream_t)stream);
        if (rc >= 0) return rc;
    }
    return dispatch_gemm(g, 0, splits, (hipStream_t)stream);
}


// ------------------------------------------------------------------------------------------
// 3x3 convolution: which kernel takes a shape
// ------------------------------------------------------------------------------------------
// Every knob of the choice, read once.  Selection knobs (both builds: the parity tests force them) — OCR_CONV_WS: 0 never conv_ws, 1 (default)
// where a workgroup gets at least two tiles, 2 every shape it covers; OCR_CONV_K2 = 0: neither conv_k2 nor conv_k3; OCR_CONV_K3 = 0: no conv_k3;
// OCR_K2_CFG = A / D: that tile wherever it covers the shape.  The others are tuning knobs (ocr_tune_env: experiments builds only).
struct ConvKnobs {
    int ws, k2, k3, k2_cfg;
    int k2_minsteps, k2_mintiles, k2_allow_a, k2_abl, k2_nst;
    int k3_minsteps, k3_genw, k3_prio;
    int halo_nw, halo_stagger, halo_stagger_bit, halo_prio;
};
static int env_int(const char* e, int dflt) { return e ? atoi(e) : dflt; }
static ConvKnobs read_conv_knobs() {
    ConvKnobs k;
    k.ws = env_int(getenv("OCR_CONV_WS"), 1);
    // conv_k2 / conv_k3 on since conv_k2's weight prefetch distance went from 2 to 3 steps (profiles/r03n: the step 1.415 against 1.440 ms, three
    // interleaved runs each; with distance 2 it was an opt-in: no faster (tile D) or 1.4 % slower (tiles A + D) in the step,
    // profiles/r03l_bench_conv_ab.log, although 8 % faster back to back, profiles/r03j_conv_k2_final.log)
    k.k2 = env_int(getenv("OCR_CONV_K2"), 1);
    k.k3 = env_int(getenv("OCR_CONV_K3"), 1);
    const char* cfg = getenv("OCR_K2_CFG");
    k.k2_cfg = (cfg && (cfg[0] == 'A' || cfg[0] == 'D')) ? cfg[0] : 0;
    k.k2_minsteps = env_int(ocr_tune_env("OCR_K2_MINSTEPS"), 18);
    k.k2_mintiles = env_int(ocr_tune_env("OCR_K2_MINTILES"), 128);
    const char* tiles = ocr_tune_env("OCR_K2_TILES");    // = D: never tile A (see k2_tile)
    k.k2_allow_a = !(tiles && tiles[0] == 'D');
    k.k2_abl = env_int(ocr_tune_env("OCR_K2_ABL"), 0);   // conv_k2's timing ablations (wrong results) and stamps
    k.k2_nst = env_int(ocr_tune_env("OCR_K2_NST"), 0);   // conv_k2's weight stages (prefetch distance + 2); 0: per tile as measured
    // conv_k3's own step floor (default 18 like conv_k2: the 9-step conv2 forward is no faster on it than on conv_halo's two workgroups per CU —
    // 34.0 against 33.6 us, 41 against 39.7 behind a cache scrub, profiles/r03t)
    k.k3_minsteps = env_int(ocr_tune_env("OCR_K3_MINSTEPS"), 18);
    k.k3_genw = env_int(ocr_tune_env("OCR_K3_GENW"), 1);                 // 0: general-width shapes stay on conv_k2 / conv_halo
    k.k3_prio = env_int(ocr_tune_env("OCR_K3_PRIO"), 2);                 // measured: 1 (equal) 349 us, 2 322, 3 324 over the ten layers (profiles/r03af)
    k.halo_nw = env_int(ocr_tune_env("OCR_HALO_NW"), 0);                 // 8 / 4 force one workgroup size, unset = by grid size
    const char* st = ocr_tune_env("OCR_HALO_STAGGER");   // units[,bit]: workgroups whose in-XCD index has `bit` set start units x 64 clocks late
    const char* comma = st ? strchr(st, ',') : nullptr;
    k.halo_stagger = st && atoi(st) > 0 ? atoi(st) : 0;
    k.halo_stagger_bit = comma ? atoi(comma + 1) : 32;
    k.halo_prio = env_int(ocr_tune_env("OCR_HALO_PRIO"), 1);             // measured: 451 against 458 us over the ten launches
    return k;
}
static const ConvKnobs& conv_knobs() {
    static const ConvKnobs k = read_conv_knobs();
    return k;
}

// CU count of the device: latched only once the query SUCCEEDED (the host-only plan queries of the lowering — possibly no device
// at all — came first and fixed the 256 fallback for the rest of the process); until then every call asks again
int ocr_cu_count() {
    static int cus = 0;
    if (!cus) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    }
    return cus > 0 ? cus : 256;                          // no device visible (CPU-only policy tests): the MI355X's count
}

// conv_ws (weights in registers, workgroups persistent over the pixel tiles) for the short-K layers it covers
static bool plan_ws(ConvPlan& p, const ConvKnobs& k) {
    if (!k.ws || (p.flags & ~(EPI_BIAS | EPI_RELU | EPI_MASK))) return false;
    if (p.epi_kind && (!(p.flags & EPI_RELU) || (p.flags & EPI_MASK))) return false;
    if ((p.Cout & 63) || (long)p.M * p.Cin * 2 > 0x7fffffffL || (long)p.M * p.Cout * 2 > 0x7fffffffL) return false;
    int nc, bm;
    if (p.H == 16 && p.Cin == 64) { nc = 16; bm = 256; }
    else if (p.H == 16 && p.Cin == 128) { nc = 8; bm = 128; }
    else if (p.H == 8 && p.Cin == 128) { nc = 16; bm = 128; }
    else return false;
    if (p.W % nc || p.M % bm || (p.epi_kind == CONV_EPI_POOL22 && (p.W & 1))) return false;
    const int ncu = ocr_cu_count();
    // default policy (measured, profiles/r05e_ws_bench.log): the single-chunk instance (Cin = 64: conv2 forward 40.8 -> 32.3 us) from two tiles
    // per workgroup on; the K-split instances (Cin = 128) are correct but lose to conv_k3 (conv2 data gradient 35 against 28 us, conv3_1 forward
    // 32 against 21: their per-workgroup weight hand-round costs 7-8 us of a 4-tile run) — OCR_CONV_WS=2 runs them for the parity tests
    const int mtiles = p.M / bm, ntiles = p.Cout / 64;
    if (k.ws == 1 && (p.Cin != 64 || (long)mtiles * ntiles < 2L * ncu)) return false;
    int slots = ncu / ntiles;
    if (slots < 1) slots = 1;
    if (slots > mtiles) slots = mtiles;
    p.per_slot = (mtiles + slots - 1) / slots;
    p.slots = (mtiles + p.per_slot - 1) / p.per_slot;    // no idle workgroups behind the last tile
    p.grid = p.slots * ntiles;
    p.xcd_map = (p.grid % 8 == 0 && (p.grid / 8) % ntiles == 0) ? 1 : 0;
    p.family = CONV_WS; p.ws_nc = nc; p.ws_ksplit = p.Cin == 64 ? 1 : 2;
    return true;
}

// conv_k2 / conv_k3's tile, if any: A (256 x 128) where its tiles fill the chip (>= 224), else D (256 x 64); layers with fewer than
// `minsteps` K steps stay on conv_halo: with 9 steps a tile is mostly prologue and epilogue, and conv_halo's two independent workgroups per
// CU overlap those (measured: conv2 33 against 40 us; conv3_1 forward, 18 steps: 26.9 on conv_halo, 27.6 on conv_k2, 24.0 on conv_k3 —
// profiles/r03q).  OCR_K2_CFG = A / D forces one tile where it covers the shape.
static char k2_tile(const ConvPlan& p, const ConvKnobs& k, int minsteps) {
    const long M = p.M;
    if ((p.Cin & 63) || (p.Cout & 63) || M < 4096 || p.H > 16 || p.H < 1) return 0;
    if (M * p.Cin * 2 >= 0x7fffffffL || (long)p.Cout * 9 * p.Cin * 2 >= 0x7fffffffL) return 0;   // 32-bit descriptor offsets
    // OCR_K2_TILES = D keeps the choice off tile A.  With prefetch distance 2 tile A was SLOWER than conv_halo inside the train step
    // (1.461 against 1.435 ms, profiles/r03k) and 15-25 % slower behind a cache scrub (profiles/r03m) although 6 % faster when the same
    // launch repeats back to back: one 8-wave workgroup per CU in lock step has nothing to run while a piece arrives late from HBM.
    // With distance 3 (five weight stages) it is faster in all three settings (profiles/r03n: cold 474 against 504 us over the ten
    // layers, hot 416 against 446, step 1.415 against 1.440 ms).
    // First a tile whose grid fills the chip (>= 224 workgroups: A, then D), else one that fills at least half of it (OCR_K2_MINTILES, 128:
    // the small-batch layers of configs[4], 6090 -> 6513 images/s; for the headline net preferring A with 128 tiles over D with 256 cost
    // 22 us per step, profiles/r03_final_a_* against r03y)
    for (int pass = 0; pass < 2; ++pass)
        for (const char c : {'A', 'D'}) {
            if (k.k2_cfg && c != k.k2_cfg) continue;
            if (!k.k2_cfg && c == 'A' && !k.k2_allow_a) continue;
            const int bn = c == 'A' ? 128 : 64;
            if (p.Cout % bn) continue;
            if (k.k2_cfg) return c;
            if (9 * (p.Cin / 64) < minsteps) return 0;
            if ((M + 255) / 256 * (p.Cout / bn) >= (pass == 0 ? 224 : k.k2_mintiles)) return c;
        }
    return 0;
}

// conv_k3 (conv_k2's tiles with the halo stored as feature-row planes) with the tile k2_tile chose: where its instances cover the shape
static bool plan_k3(ConvPlan& p, const ConvKnobs& k, char tile) {
    const int H = p.H, epi = p.epi_kind;
    if (H != 2 && H != 4 && H != 8 && H != 16) return false;
    if (p.M % 256 || (p.Cin & 63) || (p.Cout & 63) || (tile == 'A' && p.Cout % 128)) return false;
    const int NC = 256 / H, PS = (NC + 2 + 7) / 8 * 8;
    const bool genw = p.W % NC != 0;                     // tiles cross image boundaries: the general-width form (one zero row per boundary)
    if (genw && (H == 16 || NC + 2 + (NC + p.W - 1) / p.W > PS)) return false;     // (H = 16: 16-column tiles, W >= 16 there — not instantiated)
    if (genw && !k.k3_genw) return false;
    if (H == 2 && (!genw || epi == CONV_EPI_POOL12 || epi == CONV_EPI_POOL22)) return false;  // H = 2: the general-width form only (128-column tiles)
    if (epi >= CONV_EPI_STATS && (p.flags & EPI_ACCUM)) return false;    // statistics are taken in the staged write-out
    // batch-norm backward sums: of the ReLU-masked gradient; instances exist for the shapes batch-norm layers have here: H in {4, 8}, several chunks
    if (epi == CONV_EPI_BNBWD && (!(p.flags & EPI_MASK) || p.Cin == 64 || (H != 4 && H != 8))) return false;
    p.family = CONV_K3; p.tile = tile; p.genw = genw; p.single = H == 16 && p.Cin == 64; p.prio = k.k3_prio;
    return true;
}

// conv_k3 where it covers the shape (its own step floor; OCR_CONV_K3 = 0: never), else conv_k2 (128 x 64 wave tiles through an in-workgroup
// K split) where its tiles fill the chip
static bool plan_k3_k2(ConvPlan& p, const ConvKnobs& k) {
    if (k.k3) {
        const char t = k2_tile(p, k, k.k3_minsteps >= 0 ? k.k3_minsteps : k.k2_minsteps);
        if (t && plan_k3(p, k, t)) return true;
    }
    if (p.epi_kind >= CONV_EPI_STATS) return false;      // batch-norm sums in the epilogue: conv_k3 only
    const char t = k2_tile(p, k, k.k2_minsteps);
    if (!t) return false;
    // tile A: five weight stages = prefetch distance 3 (see k2_tile); tile D: four — five or six change nothing for it (profiles/r03o)
    int nst = t == 'A' ? 5 : 4;
    if ((t == 'A' && k.k2_nst == 4) || (t == 'D' && (k.k2_nst == 5 || k.k2_nst == 6))) nst = k.k2_nst;
    const int FM = t == 'A' ? 8 : 4, BN = t == 'A' ? 128 : 64;
    const int NRpad = (256 + 2 * p.H + 4 + 7) / 8 * 8;  // = launch_k2: needed rows + two zero rows, in 8-row DMA pieces
    const int lds = 2 * NRpad * 128 + nst * BN * 128;
    if (lds > 163840 || lds < 8 * FM * 2048) return false;
#ifdef OCR_EXPERIMENTS
    if (lds + 10240 > 163840 && (k.k2_abl & 8)) return false;   // no room for the stamps
#endif
    p.family = CONV_K2; p.tile = t; p.nst = nst; p.abl = k.k2_abl;
    return true;
}

// conv_halo (lock-step tap reuse).  128-pixel workgroups of 4 waves leave room for TWO workgroups per CU (80 KiB of LDS each): they drift out
// of phase, so one's MFMA burst covers the other's barrier / DMA-issue / LDS-read phase (+5-7 % where the grid then still has two workgroups
// for every CU).  Otherwise 256-pixel workgroups of 8 waves, one per CU.
static bool plan_halo(ConvPlan& p, const ConvKnobs& k) {
    const int H = p.H, Cout = p.Cout, nw = k.halo_nw;
    p.prio = k.halo_prio; p.stagger = k.halo_stagger; p.stagger_bit = k.halo_stagger_bit;
    if (nw != 8) {
        const int NR = 128 + 2 * H + 2, NRp = (NR + 32) / 32 * 32;
        const long mt4 = (p.M + 127) / 128;
        if (NRp / 32 == 5 || NRp / 32 == 6) {            // counted vmcnt literals exist for 5 and 6
            // otherwise the smallest tile: it has the most workgroups, and every alternative below leaves CUs idle (a 256-channel
            // layer at M = 8192 is 256 workgroups here against 64 of the 8-wave 256 x 128 tile)
            p.family = CONV_HALO; p.nw = 4; p.bn = (Cout >= 128 && mt4 * ((Cout + 127) / 128) >= 448) ? 128 : 64;
            return true;
        }
        if (nw == 4) return false;
    }
    const int NRpad = (256 + 2 * H + 2 + 64) / 64 * 64;
    if (NRpad / 64 != 5 && NRpad / 64 != 6) return false;
    const long mt = (p.M + 255) / 256;
    p.family = CONV_HALO; p.nw = 8;
    p.bn = (Cout >= 128 && (mt * ((Cout + 127) / 128) >= 200 || mt * ((Cout + 63) / 64) < 256)) ? 128 : 64;
    return true;
}

// The unpool write-outs (a data gradient routed through the max-pool in front): exactly where the aligned-width conv_k3 instances take the
// shape — the CODES instances' coverage (no general width, no accumulate, no mask), H in {4, 8}: whole 256-pixel tiles inside one image, whole
// channel tiles.  The tile is the plain data gradient's where that runs an aligned-width conv_k3 (the same instance with another write-out:
// the same bits); a shape below the tap-reuse kernels' size floor takes A where the channels allow it, else D.
static void plan_unpool(ConvPlan& p, const ConvKnobs& k) {
    const int H = p.H;
    if (!k.k2 || !k.k3 || p.flags || (H != 4 && H != 8) || p.M <= 0 || p.M % 256 || p.W % (256 / H) || (p.Cin & 63) || (p.Cout & 63)) return;
    if ((long)p.M * p.Cin * 2 >= 0x7fffffffL || (long)p.Cout * 9 * p.Cin * 2 >= 0x7fffffffL) return;      // 32-bit descriptor offsets
    const ConvPlan plain = conv3x3_plan(p.M, p.W, H, p.Cin, p.Cout, 0, CONV_EPI_PLAIN);
    p.tile = (plain.family == CONV_K3 && !plain.genw) ? plain.tile : ((p.Cout % 128) ? 'D' : 'A');
    p.family = CONV_K3; p.genw = false; p.single = false; p.prio = k.k3_prio;
}

ConvPlan conv3x3_plan(int M, int W, int H, int Cin, int Cout, int flags, int epi_kind) {
    const ConvKnobs& k = conv_knobs();
    ConvPlan p = {};
    p.family = CONV_GEMM; p.M = M; p.W = W; p.H = H; p.Cin = Cin; p.Cout = Cout; p.flags = flags; p.epi_kind = epi_kind;
    if (epi_kind == CONV_EPI_UNPOOL12 || epi_kind == CONV_EPI_UNPOOL22) {
        if (g_use_halo) plan_unpool(p, k);
        return p;
    }
    if (!g_use_halo || (Cin & 63) || (Cout & 3) || M < 1024 || H > 30) return p;
    if (flags & ~(EPI_BIAS | EPI_RELU | EPI_MASK | EPI_ACCUM)) return p;
    if (epi_kind < CONV_EPI_STATS && plan_ws(p, k)) return p;
    if (epi_kind >= CONV_EPI_STATS) {   // batch-norm sums from the epilogue: the plane-layout kernels only
        if (epi_kind > CONV_EPI_BNBWD || (flags & EPI_ACCUM) || (M & 255)) return p;
        if (epi_kind == CONV_EPI_STATS ? (flags & EPI_MASK) != 0 : !(flags & EPI_MASK)) return p;
        if (k.k2) plan_k3_k2(p, k);
        return p;
    }
    if (epi_kind) {     // fused max-pool: ReLU epilogue without mask, even feature axis, 2 x 2 only for H in {4, 8, 16} and even W
        if ((flags & (EPI_MASK | EPI_ACCUM)) || !(flags & EPI_RELU) || (H & 1) || (Cout % 64)) return p;
        if (epi_kind == CONV_EPI_POOL22 && ((H != 4 && H != 8 && H != 16) || (W & 1))) return p;
        if (epi_kind != CONV_EPI_POOL12 && epi_kind != CONV_EPI_POOL22) return p;
        if (M % (epi_kind == CONV_EPI_POOL22 ? 2 * H : 2)) return p;
    }
    if (k.k2 && plan_k3_k2(p, k)) return p;
    plan_halo(p, k);
    return p;
}

static int conv3x3_launch(const ConvPlan& p, const ConvOperands& o, hipStream_t stream) {
    switch (p.family) {
    case CONV_WS: return launch_ws(p, o, stream);
    case CONV_K3: return launch_k3(p, o, stream);
    case CONV_K2: return launch_k2(p, o, stream);
    case CONV_HALO: return launch_halo(p, o, stream);
    }
    return OCR_ERR_INVALID;
}
// the product's pixel count as a plan input (0: out of range, no convolution kernel)
static int conv3x3_pixels(int Nb, int W, int H, int Cin, int Cout) {
    const long M = (long)Nb * W * H;
    return (Nb <= 0 || W <= 0 || H <= 0 || Cin <= 0 || Cout <= 0 || M > 0x7fffffffL) ? 0 : (int)M;
}

// flags may carry OCR_EPI_ACCUM (y += result, bf16) only where this returns non-zero (the tap-reuse kernels' epilogues)
extern "C" int ocr_conv3x3_accum_supported(int Nb, int W, int H, int Cin, int Cout) {
    return conv3x3_plan(conv3x3_pixels(Nb, W, H, Cin, Cout), W, H, Cin, Cout, EPI_ACCUM, CONV_EPI_PLAIN).family != CONV_GEMM;
}
// Which kernel family ocr_conv3x3_bf16 / ocr_conv3x3_relu_pool_bf16 would run for this shape (host-only: nothing is launched, no GPU is
// needed): 0 the generic GEMM engines (igemm / gemm), 1 conv_halo, 2 / 3 conv_k2 tile A (256 x 128) / D (256 x 64), 4 / 5 conv_k3 A / D,
// 6 / 7 conv_k3w (general width) A / D, 8 conv_ws (weight-stationary persistent); -OCR_STATUS_INVALID (negative) for non-positive sizes.  flags as for ocr_conv3x3_bf16; (kw, kh) = (0, 0) or the window of a fused max-pool.
extern "C" int ocr_conv3x3_kernel_choice(int Nb, int W, int H, int Cin, int Cout, int flags, int kw, int kh) {
    if (Nb <= 0 || W <= 0 || H <= 0 || Cin <= 0 || Cout <= 0) return -OCR_ERR_INVALID;      // negative: 0..8 are kernel families
    const int pool_kind = (kw == 1 && kh == 2) ? 1 : ((kw == 2 && kh == 2) ? 2 : 0);
    if ((kw || kh) && !pool_kind) return 0;
    return conv3x3_plan(Nb * W * H, W, H, Cin, Cout, flags & ~(EPI_ATOMIC | EPI_ROWSWAP), pool_kind).choice();
}

// 3x3 SAME stride-1 convolution over the reference layout [Nb, W, H, C] as an implicit GEMM.
// wpack is [Cout][3][3][Cin] bf16 (K-contiguous rows).  Used for the forward (wpack = packed
// weights) and for dgrad (x := dY, wpack := flipped/transposed weights, Cin/Cout swapped).
extern "C" int ocr_conv3x3_bf16(const void* x, const void* wpack, void* y, int Nb, int W, int H,
                                int Cin, int Cout, const float* bias, const void* mask, int flags,
                                void* stream) {
    GemmArgs g = {};
    g.P = (const bf16_t*)x; g.Q = (const bf16_t*)wpack; g.ldp = Cin; g.ldq = 9L * Cin;
    g.M = Nb * W * H; g.N = Cout; g.K = 9 * Cin; g.cW = W; g.cH = H; g.cC = Cin;
    g.out = y; g.ldo = Cout; g.bias = bias; g.mask = (const bf16_t*)mask; g.ldmask = Cout;
    g.flags = flags & ~(EPI_ATOMIC | EPI_ROWSWAP);
    if ((flags & EPI_BIAS) && !bias) return OCR_ERR_INVALID;
    if ((flags & EPI_MASK) && !mask) return OCR_ERR_INVALID;
    if ((flags & EPI_ACCUM) && !ocr_conv3x3_accum_supported(Nb, W, H, Cin, Cout)) return OCR_ERR_INVALID;      // bf16 accumulate: tap-reuse epilogues only
    if (!x || !wpack || !y || g.M <= 0 || Cout <= 0 || Cin <= 0) return dispatch_gemm(g, 1, 1, (hipStream_t)stream);
    const ConvPlan p = conv3x3_plan(g.M, W, H, Cin, Cout, g.flags, CONV_EPI_PLAIN);
    if (p.family != CONV_GEMM) return conv3x3_launch(p, {x, wpack, y, bias, mask}, (hipStream_t)stream);
    if (g_use_igemm) {
        int rc = ig_try_dispatch(x, Cin, wpack, 9L * Cin, y, Cout, g.M, Cout, 9 * Cin, bias, mask, Cout, g.flags, 1, 0, 0, W, H, Cin,
                                 0, 0, (hipStream_t)stream);
        if (rc >= 0) return rc;
    }
    return dispatch_gemm(g, 1, 1, (hipStream_t)stream);
}
// conv3x3 (+ bias, optional ReLU) that also leaves the batch-norm statistics of its output behind (network.py:173-178: conv -> bias ->
// batch_norm): partials = float [rows][2][Cout], rows = ocr_conv3x3_stats_rows(...) = Nb*W*H / 256 — per 256-pixel tile the per-channel sum
// and sum of squares of the bf16 values that were stored.  ocr_bn_train_fwd2(partial_rows = rows) finishes from them without reading the
// tensor for a statistics pass.  Only where the plane-layout kernels (conv_k3 / conv_k3w) take the shape: the query returns 0 otherwise
// and the call OCR_STATUS_INVALID (the caller then runs ocr_conv3x3_bf16 + the three-pass batch norm).
extern "C" int ocr_conv3x3_stats_rows(int Nb, int W, int H, int Cin, int Cout, int flags) {
    const int M = conv3x3_pixels(Nb, W, H, Cin, Cout);
    return conv3x3_plan(M, W, H, Cin, Cout, flags & ~(EPI_ATOMIC | EPI_ROWSWAP), CONV_EPI_STATS).family != CONV_GEMM ? M / 256 : 0;
}
extern "C" int ocr_conv3x3_bf16_stats(const void* x, const void* wpack, void* y, int Nb, int W, int H, int Cin, int Cout, const float* bias,
                                      int flags, float* partials, void* stream) {
    if (!x || !wpack || !y || !partials || ((flags & EPI_BIAS) && !bias) || !ocr_conv3x3_stats_rows(Nb, W, H, Cin, Cout, flags)) return OCR_ERR_INVALID;
    const ConvPlan p = conv3x3_plan(Nb * W * H, W, H, Cin, Cout, flags & ~(EPI_ATOMIC | EPI_ROWSWAP), CONV_EPI_STATS);
    return conv3x3_launch(p, {x, wpack, y, bias, nullptr, partials}, (hipStream_t)stream);
}
// The data gradient of a convolution whose INPUT came from a batch-norm + ReLU layer (network.py:176-182 -> the next conv_single): dx = (y > 0) ?
// conv3x3(dy, flipped weights) : 0 as ocr_conv3x3_bf16 with OCR_EPI_MASK writes it, and in the same epilogue the two per-channel sums the
// batch-norm backward pass of that producer needs — partials [rows][2][Cout] = (sum dx, sum dx * xhat) per 256-pixel tile, xhat = (z - mean) *
// rstd of the producer's pre-normalisation output z.  ocr_bn_train_bwd2(partial_rows = rows, premasked) finishes from them: no statistics
// pass over (z, y, dy), no second read of y.  rows = ocr_conv3x3_bnbwd_rows(...) (0: not covered - use the separate passes).
extern "C" int ocr_conv3x3_bnbwd_rows(int Nb, int W, int H, int Cin, int Cout) {
    const int M = conv3x3_pixels(Nb, W, H, Cin, Cout);
    return conv3x3_plan(M, W, H, Cin, Cout, EPI_MASK, CONV_EPI_BNBWD).family != CONV_GEMM ? M / 256 : 0;
}
extern "C" int ocr_conv3x3_dgrad_bnbwd_bf16(const void* dy, const void* wdgrad, void* dx, int Nb, int W, int H, int Cin, int Cout, const void* mask_y,
                                            const void* z, const float* mean, const float* rstd, float* partials, void* stream) {
    if (!dy || !wdgrad || !dx || !mask_y || !z || !mean || !rstd || !partials || !ocr_conv3x3_bnbwd_rows(Nb, W, H, Cin, Cout)) return OCR_ERR_INVALID;
    const ConvPlan p = conv3x3_plan(Nb * W * H, W, H, Cin, Cout, EPI_MASK, CONV_EPI_BNBWD);
    return conv3x3_launch(p, {dy, wdgrad, dx, nullptr, mask_y, partials, z, mean, rstd}, (hipStream_t)stream);
}
// conv3x3 + bias + ReLU with the max-pool that follows it (LSTM_train.py:26-33: conv2 -> pool2 2 x 2, conv3_2 / conv4_2 -> 1 x 2
// over the feature axis) written by the same epilogue: y (kept for the backward pass) AND pooled.  kw = window along W (time),
// kh = window along H (feature): (1, 2) or (2, 2).  Only the tap-reuse kernels have this epilogue: OCR_ERR_INVALID when the shape is
// not covered (ocr_conv3x3_pool_supported tells beforehand) - the caller then runs ocr_conv3x3_bf16 + ocr_maxpool_fwd.
static int conv3x3_pool_kind(int kw, int kh) { return (kw == 1 && kh == 2) ? 1 : ((kw == 2 && kh == 2) ? 2 : 0); }
extern "C" int ocr_conv3x3_pool_supported(int Nb, int W, int H, int Cin, int Cout, int kw, int kh) {
    const int kind = conv3x3_pool_kind(kw, kh);
    return kind && conv3x3_plan(conv3x3_pixels(Nb, W, H, Cin, Cout), W, H, Cin, Cout, EPI_BIAS | EPI_RELU, kind).family != CONV_GEMM;
}
extern "C" int ocr_conv3x3_relu_pool_bf16(const void* x, const void* wpack, void* y, void* pooled, int Nb, int W, int H, int Cin,
                                          int Cout, const float* bias, int kw, int kh, void* stream) {
    if (!x || !wpack || !y || !pooled || !bias || !ocr_conv3x3_pool_supported(Nb, W, H, Cin, Cout, kw, kh)) return OCR_ERR_INVALID;
    const ConvPlan p = conv3x3_plan(Nb * W * H, W, H, Cin, Cout, EPI_BIAS | EPI_RELU, conv3x3_pool_kind(kw, kh));
    return conv3x3_launch(p, {x, wpack, y, bias, nullptr, pooled}, (hipStream_t)stream);
}
// The training form of that launch: the pool's routing codes — uint32 [Nb * W/kw * H/kh][Cout / 8], 4 bits per channel: index of the window's
// first maximum in TF scan order | (maximum > 0) << 2, compared on the bf16 values of y (ocr_maxpool_bwd_codes routes the gradient with them,
// bit-identical to ocr_maxpool_bwd on y) — are written by the same epilogue, and y may be NULL: then the full-resolution tensor is not stored
// at all.  Only conv_ws and the aligned-width conv_k3 instances have the form: ocr_conv3x3_pool_codes_supported tells whether the kernel planned
// for the shape does (0: run ocr_conv3x3_relu_pool_bf16 and keep y for ocr_maxpool_bwd).
static bool conv3x3_plan_has_codes(const ConvPlan& p) { return p.family == CONV_WS || (p.family == CONV_K3 && !p.genw); }
extern "C" int ocr_conv3x3_pool_codes_supported(int Nb, int W, int H, int Cin, int Cout, int kw, int kh) {
    const int kind = conv3x3_pool_kind(kw, kh);
    return kind && conv3x3_plan_has_codes(conv3x3_plan(conv3x3_pixels(Nb, W, H, Cin, Cout), W, H, Cin, Cout, EPI_BIAS | EPI_RELU, kind));
}
// The data gradient of the convolution BEHIND such a pool with the pool's backward pass in its write-out: conv3x3(dy, wdgrad) at the pooled
// resolution [Nb, W, H], stored only as the gradient of the pool's input out_full [Nb, W * kw, H * kh, Cout], routed by the codes of the pool
// ([Nb * W * H][Cout / 8]) as ocr_maxpool_bwd_codes routes it.  Host-only query first: 0 = not covered, run ocr_conv3x3_bf16 + ocr_maxpool_bwd_codes.
static int conv3x3_unpool_kind(int kw, int kh) { return (kw == 1 && kh == 2) ? CONV_EPI_UNPOOL12 : ((kw == 2 && kh == 2) ? CONV_EPI_UNPOOL22 : 0); }
extern "C" int ocr_conv3x3_unpool_supported(int Nb, int W, int H, int Cin, int Cout, int kw, int kh) {
    const int kind = conv3x3_unpool_kind(kw, kh);
    return kind && conv3x3_plan(conv3x3_pixels(Nb, W, H, Cin, Cout), W, H, Cin, Cout, 0, kind).family == CONV_K3;
}
extern "C" int ocr_conv3x3_dgrad_unpool_bf16(const void* dy, const void* wdgrad, void* out_full, const void* codes, int Nb, int W, int H, int Cin,
                                             int Cout, int kw, int kh, int relu_mask, void* stream) {
    if (!dy || !wdgrad || !out_full || !codes || ((size_t)codes & 3) || ((size_t)out_full & 15) || !ocr_conv3x3_unpool_supported(Nb, W, H, Cin, Cout, kw, kh))
        return OCR_ERR_INVALID;
    const ConvPlan p = conv3x3_plan(Nb * W * H, W, H, Cin, Cout, 0, conv3x3_unpool_kind(kw, kh));
    return conv3x3_launch(p, {dy, wdgrad, out_full, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (void*)codes, relu_mask ? 1 : 0}, (hipStream_t)stream);
}
extern "C" int ocr_conv3x3_relu_pool_codes_bf16(const void* x, const void* wpack, void* y, void* pooled, void* codes, int Nb, int W, int H,
                                                int Cin, int Cout, const float* bias, int kw, int kh, void* stream) {
    if (!x || !wpack || !pooled || !codes || ((size_t)codes & 3) || !bias || !ocr_conv3x3_pool_codes_supported(Nb, W, H, Cin, Cout, kw, kh))
        return OCR_ERR_INVALID;
    const ConvPlan p = conv3x3_plan(Nb * W * H, W, H, Cin, Cout, EPI_BIAS | EPI_RELU, conv3x3_pool_kind(kw, kh));
    return conv3x3_launch(p, {x, wpack, y, bias, nullptr, pooled, nullptr, nullptr, nullptr, codes}, (hipStream_t)stream);
}
