// 3x3 SAME implicit-GEMM convolution with TAP REUSE for gfx950 (third generation; same contract as
// ocr_conv3x3_bf16 — reference lib/networks/network.py:160-191 forward, and its data gradient).
//
// igemm.hip streams a fresh 256-pixel x 64-channel activation tile for every (tap, channel chunk): the same
// activation rows cross L2 -> LDS nine times, and PMC shows the kernel limited by that on-chip traffic, not by
// MFMA (46 % pipe utilisation at 1 PFLOP/s).  Here a workgroup stages, per 64-channel chunk, ONE halo tile: the
// 256 output pixels are a contiguous run of the flat pixel index, and every tap of every one of them lies in the
// contiguous run [m0 - H - 1, m0 + 256 + H + 1) — so 256 + 2H + 2 rows of 128 B are DMA'd once and the nine taps
// are nine shifted views of that LDS image.  Per step (tap, chunk) only the 16 KiB weight tile is new:
// 20 KiB of LDS-DMA per 32 MFMAs per wave instead of 48 KiB.
// SAME-padding: whether a tap of an output pixel falls outside the image depends on (pixel, tap), so the halo
// image cannot be pre-zeroed; instead every lane carries a 9-bit validity mask per pixel fragment and selects
// zeros for the MFMA operand (4 v_cndmask per fragment).
// Pipeline: weight tiles double-buffered (one step ahead), halo tiles double-buffered (one chunk ahead, issued at
// tap 0 AFTER the weight DMA so the counted wait of tap 1 does not have to drain it), raw s_barrier per step.
#include "conv_plan.h"

enum { IGH_BIAS = 1, IGH_RELU = 2, IGH_MASK = 16, IGH_ACCUM = 64 /* out (bf16) += value: a data gradient added to what another consumer already delivered */ };

struct HaloArgs {
    const bf16_t* P; const bf16_t* Q;     // P [M pixels][C] ; Q [N][9*C]
    int M, N, C;                          // C % 64 == 0
    int cW, cH;
    bf16_t* out; const float* bias; const bf16_t* mask; int flags;
    bf16_t* pool; int pool_kind;          // max-pool of the (ReLU'd) output written by the same epilogue: 0 none, 1 feature pairs (1 x 2), 2 2 x 2
    int stagger, stagger_bit;             // experiment OCR_HALO_STAGGER=units,bit: workgroups whose in-XCD index has `bit` set start `units` x 64 clocks late
    int prio;                             // OCR_HALO_PRIO (default 1): s_setprio 1 around the MFMA clusters (guide T5)
};

__device__ u32x4 igh_zero_page[4];
// diagnostic (ocr_conv_halo_clock_debug): workgroup 0 stamps {shader-clock counter, 100 MHz wall clock} at entry and exit, so the
// tool can tell the clock the kernel really ran at (tools/clock_probe.py)
__device__ long long* g_halo_clk;
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

template <int BN, int NW /* waves per workgroup: 8 (256 pixels, one workgroup per CU) or 4 (128 pixels, two per CU) */,
          int ABL = 0 /* timing ablations (wrong results): 1 no fragment reads, 2 no DMA after the prologue, 5 neither (MFMA + barrier only) */,
          int RPW = 32 /* pixels of the tile per wave: 32, or 16 = "dense": 8 waves on a 128-pixel tile, two such workgroups per CU = 4 waves per SIMD */,
          int FNV = 4 /* 16-channel fragments per wave: 4 (64 x 64 wave tiles), or 8 = "wide": 64 x 128 wave tiles, 0.375 instead of 0.5 LDS fragment
                         reads per MFMA and half the weight DMA per flop, one 4-wave workgroup per CU */>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(FNV == 8 ? 1 : (RPW == 16 ? 4 : 2), FNV == 8 ? 1 : (RPW == 16 ? 4 : 2))))
void conv_halo_kernel(HaloArgs g, int NRpad /* halo rows rounded up to 8 * NW */) {
    constexpr int BM = RPW * NW;
    constexpr int FN = FNV;
    constexpr int WAVES_N = BN / (16 * FN), WAVES_M = NW / WAVES_N;
    constexpr int WM = BM / WAVES_M, FM = WM / 16;
    constexpr int QB = BN * 128, QI = BN / (8 * NW);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int PBYTES = NRpad * 128;
    unsigned char* pbuf0 = smem;                       // 2 halo stages
    unsigned char* qbuf0 = smem + 2 * PBYTES;          // 2 weight stages

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int H = g.cH, C = g.C;
    long long* const clk = g_halo_clk;
    if (clk && blockIdx.x == 0 && tid == 0) ocr_clk_enter(clk);
    // co-resident workgroups of a launch start in phase (their prologue DMA, K steps and epilogue stores coincide instead of
    // overlapping — the short-K layers run at half their MFMA-only rate): optional start offset for every other workgroup of a CU
    if (g.stagger > 0 && ((blockIdx.x >> 3) & g.stagger_bit))
        for (int i = 0; i < g.stagger; i += 16) __builtin_amdgcn_s_sleep(16);
    const int NR = BM + 2 * H + 2;                     // halo rows actually needed
    const int PI = NRpad / (8 * NW);                   // halo DMA instructions per wave (8 rows each)

    const int mtiles = (g.M + BM - 1) / BM, ntiles = (g.N + BN - 1) / BN;
    const int nblk = mtiles * ntiles;
    int L = blockIdx.x;
    if ((nblk & 7) == 0) L = (L & 7) * (nblk >> 3) + (L >> 3);
    const int m0 = (L / ntiles) * BM, n0 = (L % ntiles) * BN;

    const int rsub = lane >> 3;
    const int csrc = ((lane & 7) ^ rsub) * 8;          // LDS position lane&7 of row r holds source chunk (lane&7)^(r&7)
    const bf16_t* zero = (const bf16_t*)igh_zero_page;
    const long mfirst = (long)m0 - H - 1;              // flat pixel of halo row 0

    const bf16_t* qrow[QI];
#pragma unroll
    for (int j = 0; j < QI; ++j) {
        int n = n0 + (wave * QI + j) * 8 + rsub;
        qrow[j] = (n < g.N) ? g.Q + (long)n * 9 * C + csrc : nullptr;
    }
    auto load_q = [&](int k0, int buf) {               // k0 = tap*C + chunk*64
        unsigned char* sq = qbuf0 + buf * QB;
#pragma unroll
        for (int j = 0; j < QI; ++j) {
            const bf16_t* src = qrow[j] ? qrow[j] + k0 : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sq + (wave * QI + j) * 1024), 16, 0, 0);
        }
    };
    auto load_p = [&](int chunk, int buf) {
        unsigned char* sp = pbuf0 + buf * PBYTES;
        for (int j = 0; j < PI; ++j) {
            const int r = (wave * PI + j) * 8 + rsub;                // halo row (r & 7 == rsub)
            const long m = mfirst + r;
            const bf16_t* src = (r < NR && m >= 0 && m < g.M) ? g.P + m * C + chunk * 64 + csrc : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sp + (wave * PI + j) * 1024), 16, 0, 0);
        }
    };

    // per pixel-fragment validity of the nine taps (bit t set <=> tap t of this lane's pixel is inside the image)
    unsigned vmask[FM];
#pragma unroll
    for (int b = 0; b < FM; ++b) {
        const int m = m0 + wm * WM + b * 16 + (lane & 15);
        unsigned bits = 0;
        if (m < g.M) {
            const int h = m % H, w = (m / H) % g.cW;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ww = w + t / 3 - 1, hh = h + t % 3 - 1;
                if ((unsigned)ww < (unsigned)g.cW && (unsigned)hh < (unsigned)H) bits |= 1u << t;
            }
        }
        vmask[b] = bits;
    }

    f32x4 acc[FN][FM];
#pragma unroll
    for (int a = 0; a < FN; ++a)
#pragma unroll
        for (int b = 0; b < FM; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4, fx = lane & 7;
    const int nchunks = C / 64;
    const int nsteps = nchunks * 9;
    // Fragment addressing with as little per-step VALU work as possible (PMC: 2.4 VALU instructions per MFMA made the vector
    // ALU as busy as the matrix pipe, and the two do not overlap while all waves move in lock step):
    //   * SAME-padding: a lane whose pixel has no valid tap reads a 128-byte ROW OF ZEROS kept behind the tiles instead of
    //     selecting zeros into the 4 loaded registers — one v_cndmask on the address instead of four on the data;
    //   * the swizzle term ((kk*4 + fq) ^ (row & 7)) only depends on (lane, tap): row = wm*WM + b*16 + (lane&15) + shift,
    //     so it is formed once per step, the second K-half is `^ 64`, and the fragment index b is an immediate offset.
    // (the zero row is row NR of the current halo stage: rows NR .. NRpad-1 exist only as padding of the DMA geometry and
    //  are filled from the zero page with every halo tile; NRpad > NR always holds)
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;          // LDS byte address of smem (0 for dynamic LDS, kept general)
    const unsigned qfrag0 = (unsigned)(qbuf0 - smem) + (wn * (16 * FN) + frow) * 128 + ((fq ^ fx) << 4);   // + stage*QB, ^64 for kk = 1
    const unsigned prow0 = (wm * WM + frow) * 128;                                                  // + shift*128 + swizzle
    // prologue: weights of step 0, then halo of chunk 0
    load_q(0, 0);
    load_p(0, 0);
    int tap = 0, chunk = 0;
    for (int s = 0; s < nsteps; ++s) {
        // Q(s) was issued one step ago; at tap 1 the halo of the NEXT chunk was issued right after it and may stay in flight
        if (tap == 1 && chunk + 1 < nchunks) {
            if (PI == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else if (PI == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else if (PI == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // issue next step's weights, and (at tap 0) the next chunk's halo AFTER them
        {
            int ntap = tap + 1, nchunk = chunk;
            if (ntap == 9) { ntap = 0; ++nchunk; }
            if (ABL != 2 && ABL != 5) {
                if (s + 1 < nsteps) load_q(ntap * C + nchunk * 64, (s + 1) & 1);
                if (tap == 0 && chunk + 1 < nchunks) load_p(chunk + 1, (chunk + 1) & 1);
            }
        }
        const int shift = (H + 1) + (tap / 3 - 1) * H + (tap % 3 - 1);       // halo row of local pixel 0 for this tap
        const unsigned qa = qfrag0 + (s & 1) * QB;
        // the zero rows (NR and NR + 1, both spare: NR is even, NRpad a multiple of 32 above it) are read at the SAME position of
        // their 256 bytes as the real row would be: a redirected lane then uses the 4 of 64 banks the swizzle gave it, instead of
        // piling onto banks 0-3 (PMC r02: 0.15-0.20 conflict cycles per LDS-active
        // cycle at H = 4 / 8, where 1/4 resp. 1/8 of the lanes are redirected for six of the nine taps)
        const unsigned psw = (fq ^ ((frow + shift) & 7)) << 4;
        const unsigned pbase = (chunk & 1) * PBYTES + prow0 + shift * 128 + psw;
        unsigned pa[FM];
        const unsigned zoff = (chunk & 1) * PBYTES + NR * 128 + (((frow + shift) & 1) << 7) + psw;    // rows NR, NR + 1: address bits 0-7 (the bank) unchanged
#pragma unroll
        for (int b = 0; b < FM; ++b) pa[b] = ((vmask[b] >> tap) & 1u) ? pbase + b * 2048 : zoff;
        // All 16 fragment reads of the step are issued back to back as inline asm (the compiler does not count them, so it adds
        // no waits of its own), then two hand-placed counted waits: lgkmcnt(FN + FM) before the first K-half's MFMAs — its
        // fragments were issued first and LDS returns in order — and lgkmcnt(0) before the second.  hipcc's own schedule
        // interleaved small read groups with the MFMAs and drained lgkmcnt(0) five times per step.
        u32x4 afr[2][FN], bfr[2][FM];
        if (ABL == 1 || ABL == 5) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
                for (int a = 0; a < FN; ++a) asm volatile("" : "=v"(afr[kk][a]));
#pragma unroll
                for (int b = 0; b < FM; ++b) asm volatile("" : "=v"(bfr[kk][b]));
            }
        } else
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const unsigned qk = qa ^ (kk * 64);
#pragma unroll
            for (int a = 0; a < FN; ++a)
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(afr[kk][a]) : "v"(lds0 + qk), "n"(a * 2048));
#pragma unroll
            for (int b = 0; b < FM; ++b)
                asm volatile("ds_read_b128 %0, %1" : "=v"(bfr[kk][b]) : "v"(lds0 + (pa[b] ^ (kk * 64))));
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (kk == 0) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(FN + FM) : "memory");     // the second half's reads may stay in flight
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (g.prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int a = 0; a < FN; ++a)
#pragma unroll
                for (int b = 0; b < FM; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, afr[kk][a]),
                                                                        __builtin_bit_cast(bf16x8, bfr[kk][b]), acc[a][b], 0, 0, 0);
            if (g.prio && kk == 1) __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (++tap == 9) { tap = 0; ++chunk; }
    }

    // ---- epilogue (m-block outer, n-fragment inner: the stores completing a 128-B run of a pixel row are adjacent)
    const int flags = g.flags;
    f32x4 bv[FN];
#pragma unroll
    for (int a = 0; a < FN; ++a) {
        const int n = n0 + wn * (16 * FN) + a * 16 + (lane >> 4) * 4;
        bv[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if ((flags & IGH_BIAS) && n < g.N) bv[a] = *(const f32x4*)(g.bias + n);
    }
#pragma unroll
    for (int b = 0; b < FM; ++b) {
        const int m = m0 + wm * WM + b * 16 + (lane & 15);
        if (m >= g.M) continue;
#pragma unroll
        for (int a = 0; a < FN; ++a) {
            const int n = n0 + wn * (16 * FN) + a * 16 + (lane >> 4) * 4;
            if (n >= g.N) continue;
            f32x4 v = acc[a][b] + bv[a];
            if (flags & IGH_RELU) {
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
            if (flags & IGH_MASK) {
                u32x2 mk = *(const u32x2*)(g.mask + (long)m * g.N + n);
                if (!(bf_lo(mk.x) > 0.f)) v.x = 0.f;
                if (!(bf_hi(mk.x) > 0.f)) v.y = 0.f;
                if (!(bf_lo(mk.y) > 0.f)) v.z = 0.f;
                if (!(bf_hi(mk.y) > 0.f)) v.w = 0.f;
            }
            if (flags & IGH_ACCUM) {
                const u32x2 old = *(const u32x2*)(g.out + (long)m * g.N + n);
                v.x += bf_lo(old.x); v.y += bf_hi(old.x); v.z += bf_lo(old.y); v.w += bf_hi(old.y);
            }
            u32x2 pk;
            pk.x = pack_bf2(v.x, v.y);
            pk.y = pack_bf2(v.z, v.w);
            *(u32x2*)(g.out + (long)m * g.N + n) = pk;
            if (g.pool_kind) {
                // max-pool window of this pixel (max_pool after the ReLU: LSTM_train.py:27-33).  Rounding to bf16 is monotone, so
                // the max of the fp32 values, rounded, is the max of the stored bf16 values.  Feature-axis neighbour = pixel m ^ 1 =
                // lane ^ 1; time-axis neighbour = pixel m +- H: lane ^ H for H = 4, 8, the same lane of fragment b ^ 1 for H = 16.
                // (M is a multiple of 2 H, tiles start at multiples of 32 pixels: a window never straddles tiles or the m < M bound.)
                f32x4 mx = v;
                if (g.pool_kind == 2) {
                    if (H == 16) {
                        f32x4 u = acc[a][FM > 1 ? (b ^ 1) : 0] + bv[a];      // (instances with FM == 1 are not dispatched for this case)
                        u.x = fmaxf(u.x, 0.f); u.y = fmaxf(u.y, 0.f); u.z = fmaxf(u.z, 0.f); u.w = fmaxf(u.w, 0.f);
                        mx.x = fmaxf(mx.x, u.x); mx.y = fmaxf(mx.y, u.y); mx.z = fmaxf(mx.z, u.z); mx.w = fmaxf(mx.w, u.w);
                    } else {
                        mx.x = fmaxf(mx.x, __shfl_xor(mx.x, H, 64)); mx.y = fmaxf(mx.y, __shfl_xor(mx.y, H, 64));
                        mx.z = fmaxf(mx.z, __shfl_xor(mx.z, H, 64)); mx.w = fmaxf(mx.w, __shfl_xor(mx.w, H, 64));
                    }
                }
                mx.x = fmaxf(mx.x, __shfl_xor(mx.x, 1, 64)); mx.y = fmaxf(mx.y, __shfl_xor(mx.y, 1, 64));
                mx.z = fmaxf(mx.z, __shfl_xor(mx.z, 1, 64)); mx.w = fmaxf(mx.w, __shfl_xor(mx.w, 1, 64));
                const int h = m % H, col = m / H;
                const bool writer = !(h & 1) && (g.pool_kind == 1 || !(col & 1));
                if (writer) {
                    const long pidx = g.pool_kind == 1 ? (long)(m >> 1) : (long)(col >> 1) * (H >> 1) + (h >> 1);
                    u32x2 pp;
                    pp.x = pack_bf2(mx.x, mx.y);
                    pp.y = pack_bf2(mx.z, mx.w);
                    *(u32x2*)(g.pool + pidx * g.N + n) = pp;
                }
            }
        }
    }
    if (clk && blockIdx.x == 0 && tid == 0) ocr_clk_exit(clk);
}

// (A variant on v_mfma_f32_32x32x16_bf16 — same tiles, 32-row fragments, row swizzle (r & 7) ^ ((r >> 3) & 1) — was written in round 2,
// passed the parity tests on hardware in round 3 and measured 10-15 % SLOWER on every layer (profiles/r03a_conv_32x32x16.log): removed.)

template <int BN, int NW>
static int run_halo(const HaloArgs& g, hipStream_t stream) {
    constexpr int BM = 32 * NW;
    const int NR = BM + 2 * g.cH + 2;
    const int NRpad = (NR + 8 * NW) / (8 * NW) * (8 * NW);       // strictly greater than NR: the spare rows are the zero rows
    const int lds = 2 * NRpad * 128 + 2 * BN * 128;              // halo stages, weight stages
    if (ocr_allow_lds<conv_halo_kernel<BN, NW>>(lds) != hipSuccess) return OCR_ERR_EXEC;
    const int mt = (g.M + BM - 1) / BM, nt = (g.N + BN - 1) / BN;
    conv_halo_kernel<BN, NW><<<mt * nt, 64 * NW, lds, stream>>>(g, NRpad);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
// tiles: BN channels x 32 * NW pixels (conv3x3_plan's plan_halo chooses)
int launch_halo(const ConvPlan& p, const ConvOperands& o, hipStream_t stream) {
    const HaloArgs g = {(const bf16_t*)o.x, (const bf16_t*)o.wpack, p.M, p.Cout, p.Cin, p.W, p.H, (bf16_t*)o.y, o.bias, (const bf16_t*)o.mask,
                        p.flags, (bf16_t*)o.pool, p.epi_kind, p.stagger, p.stagger_bit, p.prio};
    if (p.nw == 4) return p.bn == 128 ? run_halo<128, 4>(g, stream) : run_halo<64, 4>(g, stream);
    return p.bn == 128 ? run_halo<128, 8>(g, stream) : run_halo<64, 8>(g, stream);
}

int k3_set_clock_debug(void* dbg);       // conv_k3.hip: the plane-layout kernels stamp the same block
int ws_set_clock_debug(void* dbg);       // conv_ws.hip likewise
extern "C" int ocr_conv_halo_clock_debug(void* dbg /* device int64[8] or NULL */) {
    long long* p = (long long*)dbg;
    if (k3_set_clock_debug(dbg) != OCR_OK || ws_set_clock_debug(dbg) != OCR_OK) return OCR_ERR_EXEC;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_halo_clk), &p, sizeof(p)) == hipSuccess ? OCR_OK : OCR_ERR_EXEC;
}
