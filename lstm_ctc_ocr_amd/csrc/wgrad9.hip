// Third-generation 3x3 SAME convolution weight gradient for gfx950 — all nine taps from ONE staged tile, no atomics.
//     dW[tap][ci][co] += sum_m X[m + shift(tap)][ci] * dY[m][co]          (reference: tf.gradients of network.py:166 at train.py:81)
//
// gemm_tn2.hip gives every (tap, 128 ci, 128 co) tile its own workgroup: the same dY rows cross L2 -> LDS nine times and the same
// X rows nine times (shifted), 32 KiB of LDS fill per 2.1 MFLOP — exactly the 64 B/clk/CU a CU can fill at the MFMA peak —
// and the split-M partial sums meet in fp32 atomics (20-28 MB per layer, a quarter of the kernel, and not bit-reproducible).
// Here a workgroup of 8 waves owns ALL NINE taps of a 64 ci x 64 co tile (36 864 fp32 results = 144 accumulator registers per
// lane on four of its waves, the other four hold the same tile for the other half of the pixels):
//   * per step of 128 pixels ONE halo tile of X (128 + 2H + 2 rows x 64 channels: every tap of every pixel of the step lies in
//     it, exactly as in conv_halo.hip) and ONE tile of dY (128 rows x 64 channels) are LDS-DMA'd: 34 KiB per 18.9 MFLOP, 8x
//     less fill per flop; the nine A operands are nine shifted views of the halo image, the B operand is shared by all taps;
//   * operands stay row-major [pixel][channel] (what DMA can write) and are transposed by ds_read_b64_tr_b16 on the way into
//     the MFMA (lane semantics pinned by tests/test_gpu_kernels.py::test_probe_tr16), k permutation as in gemm_tn.hip;
//     128-byte rows, 32-byte slot XOR ((row >> 1) & 3) on the DMA source chunk and on the read: any 8 consecutive rows x 32 B
//     of a 32-lane read half hit 64 distinct banks, for every tap shift;
//   * SAME padding without touching the fragment: the lane that supplies a padded element to the transposing read reads 8 zero
//     bytes from a zero block behind the stages instead.  "Pixel has no neighbour above / below" is loop invariant per lane and
//     folded into the per-tap offsets; "no neighbour column" (w = 0 / W-1) is an address select per 32-pixel block;
//   * waves (cb, kh): channel block cb = 16 ci, pixel half kh of the step; the halves are summed through LDS at the end
//     (halves the partial-sum traffic), the tile's partial result goes to a slab [split][9][Cin][Cout] with plain stores;
//   * a second kernel adds the S slabs into dW in a fixed order: deterministic, and the bias gradient (column sums of dY,
//     taken from the dY tile by the workgroups of ci tile 0) rides along.
// Covered: Cin % 64 == 0, Cout % 64 == 0, H in {2, 4, 8, 16}.  Everything else stays on gemm_tn2.hip / gemm_tn.hip.
// (Look-ahead 3 - 6, staggered and spread DMA, scalar-base DMA, AND / select padding masks and a continuous-stream schedule were
// measured equal or slower and deleted: DESIGN section 3 has their numbers and names the last commit that contains them.)
#include "common.h"
#include <stdlib.h>
#include <utility>
#include <type_traits>

struct W9Args {
    const bf16_t* X; const bf16_t* dY;       // [M][Cin], [M][Cout]
    int M, Cin, Cout, cW, cH;
    int k_per_split;                         // pixels per split, multiple of 128
    int S, T_ci, T_co, map;                  // splits; tiles; workgroup map (0 plain, 1 split = xcd (mod 8), 2 8/S XCDs per split)
    float* part;                             // [S][9][Cin][Cout]
    float* cs_part;                          // [S][Cout] or nullptr
};

__device__ u32x4 w9_zero_page[4];
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((ext_vector_type(4))) short s16x4;

constexpr int W9_NDMA = 5;                        // LDS-DMA instructions per wave and step (1 KiB each)
constexpr int W9_STAGE = 8 * W9_NDMA * 1024;      // 40 KiB: halo rows | dY rows | spare
constexpr int W9_NST = 3;
constexpr int W9_LA = 2;                          // A groups kept in flight ahead of the tap being multiplied
constexpr int W9_NSLOT = W9_LA + 1;               // A fragment registers in rotation
constexpr int W9_DMA_AT = 3;                      // tap before which the next stage's DMA is issued
constexpr unsigned W9_ZOFF = W9_NST * W9_STAGE;   // 8 KiB of zeros behind the stages
constexpr int W9_LDS = 4 * 9 * 4 * 4 * 64 * 4;    // 147 456 B: the epilogue's half-sum exchange (> 3 stages + 8 KiB zero block)

// transposing 8-byte fragment read at addr + imm; imm must fold to a constant at every call: it is the instruction's offset field
__device__ __forceinline__ void w9_tr(s16x4& dst, unsigned addr, int imm) { asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm)); }
#define W9_WAIT(n) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n) : "memory")

// ---- the LDS read stream of one step, as a compile-time table -------------------------------------------------------------
// Groups in issue (= return) order: B(block 0) | A(0,0) .. A(0,8) | B(block 1) | A(1,0) .. A(1,8); a B group is 8 reads, an A
// group 2.  Tap n = 9 kk + t consumes A(kk,t) and B(kk).  Before tap n the stream is advanced to LA groups past A(n), as far as
// the 4-bit lgkmcnt allows (at most 15 reads in flight); the wait of tap n is the number of reads younger than A(n).
constexpr int w9_gsize(int p) { return (p == 0 || p == 10) ? 8 : 2; }
constexpr int w9_gpos(int n) { return n < 9 ? 1 + n : 2 + n; }
constexpr int w9_younger(int n, int upto) { int o = 0; for (int q = w9_gpos(n) + 1; q <= upto; ++q) o += w9_gsize(q); return o; }
constexpr int w9_upto(int n, int LA) {
    int p = w9_gpos(n) + LA;
    if (p > 19) p = 19;
    const int own = n == 0 ? 10 : 2;                // reads of A(n) itself (and of B(0) at the first tap) may still be in flight
    while (own + w9_younger(n, p) > 15) --p;
    return p;
}
struct W9Tab { int upto[18]; int wait[18]; };
constexpr W9Tab w9_make_tab(int LA) {
    W9Tab t = {};
    for (int n = 0; n < 18; ++n) { t.upto[n] = w9_upto(n, LA); t.wait[n] = w9_younger(n, t.upto[n]); }
    return t;
}
constexpr W9Tab W9_TAB = w9_make_tab(W9_LA);

// f(integral_constant<int, FROM>) .. f(integral_constant<int, TO>), in order; nothing when TO < FROM.  The index reaches the body as a
// constant expression: the wait counts and LDS offsets derived from it are instruction immediates.
template <int FROM, int... I, class F>
__device__ __forceinline__ void w9_for_seq(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, FROM + I>{}), ...); }
template <int FROM, int TO, class F>
__device__ __forceinline__ void w9_for(F&& f) { w9_for_seq<FROM>(std::make_integer_sequence<int, (TO >= FROM ? TO - FROM + 1 : 0)>{}, f); }

// wait until at most `reads` LDS reads are in flight; `reads` is a table entry at a constant tap number, the switch folds to one instruction
__device__ __forceinline__ void w9_wait(int reads) {
    switch (reads) {
        case 0: W9_WAIT(0); break;   case 2: W9_WAIT(2); break;   case 4: W9_WAIT(4); break;   case 6: W9_WAIT(6); break;
        case 8: W9_WAIT(8); break;   case 10: W9_WAIT(10); break; case 12: W9_WAIT(12); break; default: W9_WAIT(14); break;
    }
}

// the MFMA block of one tap: the A fragment (two transposed reads) against the four 16-channel B fragments of the K block
__device__ __forceinline__ void w9_mfma_tap(f32x4 (&acc)[4], const s16x4& alo, const s16x4& ahi, const s16x4 (&blo)[4], const s16x4 (&bhi)[4]) {
    const u32x2 lo = __builtin_bit_cast(u32x2, alo), hi = __builtin_bit_cast(u32x2, ahi);
    const u32x4 av = {lo.x, lo.y, hi.x, hi.y};
    const bf16x8 fa = __builtin_bit_cast(bf16x8, av);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const u32x2 bl = __builtin_bit_cast(u32x2, blo[c]), bh = __builtin_bit_cast(u32x2, bhi[c]);
        const u32x4 bv = {bl.x, bl.y, bh.x, bh.y};
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, __builtin_bit_cast(bf16x8, bv), acc[c], 0, 0, 0);
    }
}

// workgroup -> (split, tile) for the three maps of W9Args::map
__device__ __forceinline__ void w9_block_decode(const W9Args& g, int b, int& split, int& tile) {
    const int T = g.T_ci * g.T_co;
    if (g.map == 1) { const int x = b & 7, q = b >> 3; split = (q / T) * 8 + x; tile = q % T; }
    else if (g.map == 2) { const int x = b & 7, q = b >> 3, G = 8 / g.S; split = x / G; tile = (x % G) * (T / G) + q; }
    else { split = b / T; tile = b % T; }
}

// Bias gradient: column sums of the dY tile.  Thread -> source chunk tid & 7 (8 channels), rows (tid >> 3) and (tid >> 3) + 64 of the tile
// ((csr + 64) >> 1 & 3 == csr >> 1 & 3: one slot XOR for both rows); w9_cs_offset is relative to the tile's first row.
__device__ __forceinline__ unsigned w9_cs_offset(int tid) {
    const int csq = tid & 7, csr = tid >> 3;
    return csr * 128 + (((((csq >> 1) ^ ((csr >> 1) & 3)) << 1) | (csq & 1)) << 4);
}
__device__ __forceinline__ void w9_cs_step(float (&cs)[8], unsigned addr) {
    u32x4 v0, v1;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v0) : "v"(addr));
    asm volatile("ds_read_b128 %0, %1 offset:8192" : "=v"(v1) : "v"(addr));
    W9_WAIT(0);
    __builtin_amdgcn_sched_barrier(0);
    cs[0] += bf_lo(v0.x) + bf_lo(v1.x); cs[1] += bf_hi(v0.x) + bf_hi(v1.x); cs[2] += bf_lo(v0.y) + bf_lo(v1.y); cs[3] += bf_hi(v0.y) + bf_hi(v1.y);
    cs[4] += bf_lo(v0.z) + bf_lo(v1.z); cs[5] += bf_hi(v0.z) + bf_hi(v1.z); cs[6] += bf_lo(v0.w) + bf_lo(v1.w); cs[7] += bf_hi(v0.w) + bf_hi(v1.w);
}
// ... and the end of the kernel: the 64 row groups meet in LDS (every tile in it is dead), 64 threads store the split's 64 channels
__device__ __forceinline__ void w9_cs_store(const W9Args& g, unsigned char* smem, const float (&cs)[8], int split, int co0, int tid) {
    float* red = (float*)smem;
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = cs[e];
    __syncthreads();
    if (tid < 64) {                                // channel tid = chunk tid >> 3, element tid & 7; 64 row groups
        float s = 0.f;
        for (int u = 0; u < 64; ++u) s += red[(u * 8 + (tid >> 3)) * 8 + (tid & 7)];
        g.cs_part[(long)split * g.Cout + co0 + tid] = s;
    }
    __syncthreads();
}

// Sum the two pixel halves and store the slab tile: waves kh = 1 hand their accumulators over through LDS ([wave][tap][c][r][lane],
// conflict free), waves kh = 0 add theirs and store.
// (Tried: meeting in LDS as a [tap][ci][co] tile image — ds_add_f32 from the second half, 16-byte slab stores by all eight
// waves: +40 us per layer, LDS float atomics are slow; the slab write is bound by its 37.7 MB anyway.)
__device__ __forceinline__ void w9_store_tile(const W9Args& g, unsigned char* smem, const f32x4 (&acc)[9][4], int split, int ci0, int co0,
                                              int cb, int kh, int lane) {
    const int g4 = lane >> 4, L = lane & 15;
    float* xch = (float*)smem + cb * (9 * 4 * 4 * 64) + lane;
    if (kh == 1) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) xch[((t * 4 + c) * 4 + r) * 64] = acc[t][c][r];
    }
    __syncthreads();
    if (kh == 0) {
        float* slab = g.part + (long)split * 9 * g.Cin * g.Cout;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ci = ci0 + cb * 16 + g4 * 4 + r, co = co0 + c * 16 + L;
                    slab[((long)t * g.Cin + ci) * g.Cout + co] = acc[t][c][r] + xch[((t * 4 + c) * 4 + r) * 64];
                }
    }
}

// The kernels' bodies are device functions of (job, workgroup index within the job): a launch may hold the workgroups of TWO layers
// (the paired kernels below), so a body never reads blockIdx itself.  The job is taken BY VALUE: through a reference the compiler reschedules
// the prologue of every single-job kernel; by value the plane kernels stay what they were up to operand order (DESIGN section 9 has the counts).
__device__ __forceinline__ void wgrad9_body(const W9Args g, int bid) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb = wave & 3, kh = wave >> 2;
    const int H = g.cH, W = g.cW;
    int split, tile;
    w9_block_decode(g, bid, split, tile);
    const int ti = tile / g.T_co, tj = tile % g.T_co;
    const int ci0 = ti * 64, co0 = tj * 64;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.M, kbeg + g.k_per_split);
    const int nsteps = kend > kbeg ? (kend - kbeg + 127) >> 7 : 0;
    const int NR = 128 + 2 * H + 2;                 // halo rows a step needs
    const int nhalo = (NR + 7) >> 3;                // DMA instructions covering them (8 rows of 128 B each)
    const int NRp = nhalo << 3;
    const bool do_cs = g.cs_part != nullptr && ti == 0;
    const bf16_t* zero = (const bf16_t*)w9_zero_page;

    // ---- DMA geometry: instruction u = wave + 8 i covers stage bytes [u KiB, (u + 1) KiB): lane -> row 8u' + (lane >> 3),
    //      LDS chunk position lane & 7, which holds SOURCE chunk q (slot XOR (row >> 1) & 3; (8u' + rr) >> 1 & 3 == rr >> 1 & 3)
    const int rr = lane >> 3, pp = lane & 7;
    const int qsrc = ((((pp >> 1) ^ ((rr >> 1) & 3)) << 1) | (pp & 1)) * 8;       // first channel of the source chunk
    const bf16_t* src[W9_NDMA];
    int pix[W9_NDMA];
#pragma unroll
    for (int i = 0; i < W9_NDMA; ++i) {
        const int u = wave + 8 * i;
        src[i] = zero; pix[i] = 0x40000000;            // spare piece: always the zero page
        if (u < nhalo) {
            const int r = 8 * u + rr;
            pix[i] = (r < NR) ? kbeg - (H + 1) + r : 0x40000000;
            src[i] = g.X + (long)(kbeg - (H + 1) + r) * g.Cin + ci0 + qsrc;
        } else if (u < nhalo + 16) {
            const int r = 8 * (u - nhalo) + rr;
            pix[i] = kbeg + r;
            src[i] = g.dY + (long)(kbeg + r) * g.Cout + co0 + qsrc;
        }
    }
    auto stage_load = [&](int step, int buf) {
        unsigned char* st = smem + buf * W9_STAGE;
#pragma unroll
        for (int i = 0; i < W9_NDMA; ++i) {
            const int u = wave + 8 * i;
            const int px = pix[i] + step * 128;
            const bf16_t* s = zero;
            if (u < nhalo) { if (px >= 0 && px < g.M) s = src[i] + (long)step * 128 * g.Cin; }
            else if (u < nhalo + 16) { if (px < kend) s = src[i] + (long)step * 128 * g.Cout; }
            __builtin_amdgcn_global_load_lds((gptr_t)s, (lptr_t)(st + u * 1024), 16, 0, 0);
        }
    };

    // ---- fragment addressing (loop invariant): lane (g4, L) supplies row 4 g4 + (L >> 2) of a 4 x 16 block, 8-byte piece L & 3
    const int g4 = lane >> 4, L = lane & 15;
    const int rowl = kh * 64 + 4 * g4 + (L >> 2);
    unsigned offA[9], offB[4];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int a0 = rowl + (H + 1) + (t / 3 - 1) * H + (t % 3 - 1);          // halo row of this lane's pixel for tap t
        offA[t] = a0 * 128 + ((cb ^ ((a0 >> 1) & 3)) << 5) + (L & 3) * 8;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) offB[c] = NRp * 128 + rowl * 128 + ((c ^ ((rowl >> 1) & 3)) << 5) + (L & 3) * 8;
    // SAME padding: the lane that SUPPLIES a padded element to the transposing read (row L >> 2 of its 4 x 16 block) reads 8 zero bytes
    // instead — an address select folded into the loop-invariant per-tap offsets: offA of such a lane is absolute (zero block
    // behind the stages) and its stage base is 0.  Nothing touches the fragment between the read and the MFMA (an AND / select
    // on the fragment made the compiler copy every fragment into one operand tuple: each copy waited for the previous tap's MFMAs —
    // measured 11 us of 75 on conv4_2).
    const int hsup = (4 * g4 + (L >> 2)) % H;                                     // feature row of the element this lane supplies (H = 2: a 4-row block spans two columns)
    const bool red_m = hsup == 0;                                                 // taps with dh = -1: no row above
    const bool red_p = hsup == H - 1;                                             // taps with dh = +1: no row below
    const unsigned zabs = lds0 + W9_ZOFF + (L & 3) * 8;                           // this lane's 8 zero bytes (offsets up to 6 KiB are added)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dh = t % 3 - 1;
        if ((dh < 0 && red_m) || (dh > 0 && red_p)) offA[t] = lds0 + W9_ZOFF + (offA[t] & 255);  // same banks as the real row (immediates are multiples of 256)
    }
    *(u32x4*)(smem + W9_ZOFF + tid * 16) = (u32x4){0, 0, 0, 0};                   // 512 threads x 16 B (visible after the first barrier)
    const int hs = H == 2 ? 1 : (H == 4 ? 2 : (H == 8 ? 3 : 4));                  // log2 H
    const int ncol = 32 >> hs;                                                   // image columns per 32-pixel block
    int wc = (kbeg >> hs) % W;                                                   // column (within its image) of the step's first pixel
    const int lc0 = (4 * g4 + (L >> 2)) >> hs, lc1 = (4 * g4 + (L >> 2) + 16) >> hs;   // column (inside a 32-pixel block) of the element this lane supplies, both reads

    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[t][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const unsigned offC = NRp * 128 + w9_cs_offset(tid);

#pragma unroll
    for (int p = 0; p < W9_NST - 1; ++p)
        if (p < nsteps) stage_load(p, p);
    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        if (step + 1 < nsteps) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(W9_NDMA) : "memory");     // the next step may stay in flight
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const unsigned sb = lds0 + cur * W9_STAGE;
        const unsigned sbm = red_m ? 0u : sb, sbp = red_p ? 0u : sb;      // stage base as seen by the dh = -1 / +1 taps

        s16x4 alo[W9_NSLOT], ahi[W9_NSLOT], blo[2][4], bhi[2][4];
        // "no neighbour column" (w == 0 for dw = -1, w == W - 1 for dw = +1) as an address select too, per 32-pixel block
        bool zl_m[2], zh_m[2], zl_p[2], zh_p[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            int cbase = wc + ((kh * 64 + kb * 32) >> hs);
            while (cbase >= W) cbase -= W;
            const bool bd = cbase == 0 || cbase + ncol >= W;          // does the block touch image column 0 or W - 1 ? (wave-uniform)
            int c0 = cbase + lc0, c1 = cbase + lc1;                   // < 2 W (the plan requires W >= 32 / H)
            if (c0 >= W) c0 -= W;
            if (c1 >= W) c1 -= W;
            zl_m[kb] = bd && c0 == 0; zh_m[kb] = bd && c1 == 0; zl_p[kb] = bd && c0 == W - 1; zh_p[kb] = bd && c1 == W - 1;
        }
        // the reads of stream position P (P, the tap number n and everything derived from them are constants once the loops below are unrolled)
        auto issue = [&](int P) __attribute__((always_inline)) {
            if (P == 0 || P == 10) {
                const int kb = P == 0 ? 0 : 1;
#pragma unroll
                for (int c = 0; c < 4; ++c) { w9_tr(blo[kb][c], sb + offB[c], kb * 32 * 128); w9_tr(bhi[kb][c], sb + offB[c], kb * 32 * 128 + 16 * 128); }
            } else {
                const int m = P < 10 ? P - 1 : P - 2, kb = m / 9, tt = m % 9;
                const unsigned sa = (tt % 3 == 0 ? sbm : (tt % 3 == 2 ? sbp : sb)) + offA[tt];
                unsigned sl = sa, sh = sa;
                if (tt / 3 == 0) { sl = zl_m[kb] ? zabs : sa; sh = zh_m[kb] ? zabs : sa; }
                if (tt / 3 == 2) { sl = zl_p[kb] ? zabs : sa; sh = zh_p[kb] ? zabs : sa; }
                w9_tr(alo[m % W9_NSLOT], sl, kb * 32 * 128); w9_tr(ahi[m % W9_NSLOT], sh, kb * 32 * 128 + 16 * 128);
            }
        };
#pragma unroll
        for (int P = 0; P < 20; ++P)
            if (P <= W9_TAB.upto[0]) issue(P);
        // A loop the optimiser unrolls, not w9_for: while it is still a loop, the DMA address arithmetic of tap W9_DMA_AT is hoisted out of it, to
        // the top of the step, as selects; written out as straight-line code it stays in front of tap W9_DMA_AT as 15 branches.
#pragma unroll
        for (int n = 0; n < 18; ++n) {
            if (n == W9_DMA_AT) {
                // the buffer of step + 2 was last read in step - 1: free since this step's barrier
                if (step + 2 < nsteps) { int nb = cur + 2; if (nb >= W9_NST) nb -= W9_NST; stage_load(step + 2, nb); }
            }
            if (n > 0) {                         // advance the read stream
#pragma unroll
                for (int P = 0; P < 20; ++P)
                    if (P > W9_TAB.upto[n - 1] && P <= W9_TAB.upto[n]) issue(P);
            }
            w9_wait(W9_TAB.wait[n]);
            __builtin_amdgcn_sched_barrier(0);
            w9_mfma_tap(acc[n % 9], alo[n % W9_NSLOT], ahi[n % W9_NSLOT], blo[n / 9], bhi[n / 9]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (do_cs) w9_cs_step(cs, sb + offC);      // (rows past kend are zero-filled)
        wc += 128 >> hs;
        while (wc >= W) wc -= W;
        cur = (cur + 1 == W9_NST) ? 0 : cur + 1;
    }
    __syncthreads();                                   // every DMA has landed and every tile is dead: LDS is reused below

    if (do_cs) w9_cs_store(g, smem, cs, split, co0, tid);
    w9_store_tile(g, smem, acc, split, ci0, co0, cb, kh, lane);
}
__global__ __launch_bounds__(512) void wgrad9_kernel(W9Args g) { wgrad9_body(g, blockIdx.x); }

// ---------------------------------------------------------------------------------------------------------------------------------
// PLANE-LAYOUT form of the kernel above (round 3; same slabs, same reduction, same results up to the summation order inside a step).
// wgrad9_kernel spends ~190 VALU instructions per wave and step beside its 72 MFMAs (per-tap address selects for the SAME padding,
// 64-bit DMA addresses with bounds tests): 4800 cycles per step against 2304 of MFMA, and VALU work does not hide behind the other
// wave's MFMAs.  As in conv_k3.hip, a step's 128 pixels are NC = 128 / H whole image columns, staged as H planes (plane h, row c' <-
// pixel (column c0 - 1 + c', feature row h); PS = NC + 2 rounded up to 8 rows per plane) and the dY rows in the same (h, column) order:
//   * the 32 pixels of an MFMA's K block are 32 columns of one plane (H = 4) or 16 columns of two planes (H = 8): tap (dw, dh) reads the
//     same rows shifted by dw in plane h + dh — a per-dw lane register (the slot XOR depends on ((c' + dw) >> 1) & 3 only) + an immediate;
//   * a plane that does not exist is read from the zero block with no select, and an MFMA whose 32 pixels are all padding is not issued
//     (H = 4: a sixth of them);
//   * image edges are the halo columns c' = 0 / NC + 1 of a step (W % NC == 0): their DMA lanes get bit 31 OR-ed into the lane offset
//     (out of range -> zeros) on the steps that start / end an image;
//   * DMA through buffer descriptors: loop-invariant 32-bit lane offsets, the step advance is a scalar offset.
// Covered: H in {4, 8}, W % (128 / H) == 0, M * C * 2 < 2^31; everything else stays on wgrad9_kernel.
__device__ long long* w9_dbg;                       // set by ocr_wgrad9_debug; read by the experiments build's W9P_PHASE stamps only
#ifdef OCR_EXPERIMENTS
// diagnostic (experiments build, ocr_wgrad9_debug): wall-clock stamps (100 MHz) of every workgroup's first thread —
// dbg[block * 8 + {0 entry, 1 K loop done, 2 column sums done, 3 slab stores issued, 4 acknowledged}] (tools/w9p_phases.py)
#define W9P_PHASE(slot) do { if (w9_dbg && threadIdx.x == 0) w9_dbg[blockIdx.x * 8 + (slot)] = wall_clock64(); } while (0)
#else
#define W9P_PHASE(slot) do { } while (0)
#endif
// GENW (round 6, configs[3]): any image width W >= NC — a step's NC columns may cross ONE image boundary: local column b of the step is the first
// column of the next image.  The planes are staged exactly as for whole-image steps (plane row 1 + c = local column c, the two halo rows); what
// differs is two elements of the contraction: the +1 tap of column b - 1 (the last column of image A) and the -1 tap of column b (the first of image
// B) must read zeros — the lanes that SUPPLY those two pixels are redirected, for that tap only, to one of the zero rows every plane carries behind
// its columns (rows NC + 2 .. PS - 1 arrive as zeros with every stage), so a fragment address stays "lane register + immediate" and nothing
// touches the DMA.  Per step: a uniform branch; in the steps that cross a boundary (40 % at W = 80, NC = 32) four compares and four selects.
// (First form, measured and replaced: conv_k3w's zero ROW inserted into the planes — the DMA lanes behind it fetch one column further left — cost
// ~45 VALU instructions per crossing step and ran conv4_2 at W = 80 in 78 us; profiles/r06h_ab_varwidth_first_form.log, r06h2_ab_varwidth.log.)
// Index algebra replayed on the CPU: tools/w9p_plane_model.py (a_fragment_rows_genw), tests/test_w9p_plane_model.py::test_general_width_boundary_redirect.
// plane holding the 16-pixel half `half` of K block kk of pixel half kh, shifted by dh; -1: the plane does not exist
constexpr int w9p_plane(int H, int kh, int kk, int dh, int half) {
    const int pl = H == 4 ? kh * 2 + kk + dh : kh * 4 + kk * 2 + half + dh;
    return pl >= 0 && pl < H ? pl : -1;
}
template <int H, bool GENW>
__device__ __forceinline__ void wgrad9p_body(const W9Args g, int bid) {
    constexpr int NC = 128 / H;                         // image columns per step
    constexpr int PS = (NC + 2 + 7) / 8 * 8;            // rows per plane (40 / 24)
    constexpr int XROWS = H * PS, XPIECES = XROWS / 8;  // 160 rows = 20 pieces / 192 rows = 24 pieces; then 128 dY rows = 16 pieces
    static_assert(XPIECES + 16 <= 8 * W9_NDMA, "a stage holds the planes and the dY tile");
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    W9P_PHASE(0);
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb = wave & 3, kh = wave >> 2;
    const int W = g.cW;
    int split, tile;
    w9_block_decode(g, bid, split, tile);
    const int ti = tile / g.T_co, tj = tile % g.T_co;
    const int ci0 = ti * 64, co0 = tj * 64;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.M, kbeg + g.k_per_split);
    const int nsteps = kend > kbeg ? (kend - kbeg) >> 7 : 0;       // M % 128 == 0: whole steps
    const bool do_cs = g.cs_part != nullptr && ti == 0;

    // ---- DMA geometry: instruction u = wave + 8 i covers stage bytes [u KiB, (u + 1) KiB): lane -> row 8u + (lane >> 3), LDS chunk
    //      position lane & 7, which holds SOURCE chunk q (slot XOR (row >> 1) & 3; PS % 8 == 0: (row >> 1) & 3 == (c' >> 1) & 3)
    const int rr = lane >> 3, pp = lane & 7;
    const int qsrc = ((((pp >> 1) ^ ((rr >> 1) & 3)) << 1) | (pp & 1)) * 8;       // first channel of the source chunk
    // descriptors: X from H pixels before the split (the first halo column), dY from the split; lane offsets are relative to those
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(g.X + ((long)kbeg - H) * g.Cin), 0,
                                                                          (int)(((long)g.M - kbeg + H) * g.Cin * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t ysrd = __builtin_amdgcn_make_buffer_rsrc((void*)(g.dY + (long)kbeg * g.Cout), 0,
                                                                          (int)(((long)g.M - kbeg) * g.Cout * 2), 0x00020000);
    // GENW: zero rows of a plane the redirected lanes read: ZLO for the first read of a tap, ZHI + 16 (H = 4: the second read carries a 16-row immediate)
    constexpr int ZLO = NC + 4, ZHI = H == 4 ? NC + 4 - 16 : NC + 4;
    static_assert(NC + 2 <= ZLO && ZLO < PS, "a zero row exists behind the columns of every plane");
    unsigned voff[W9_NDMA], eL[W9_NDMA], eR[W9_NDMA];
#pragma unroll
    for (int i = 0; i < W9_NDMA; ++i) {
        const int u = wave + 8 * i;
        voff[i] = OOB; eL[i] = 0; eR[i] = 0;           // spare piece: zeros
        if (u < XPIECES) {
            const int r = 8 * u + rr, h = r / PS, cp = r % PS;
            if (cp < NC + 2) voff[i] = (unsigned)(((cp * H + h) * g.Cin + ci0 + qsrc) * 2);
            eL[i] = cp == 0 ? OOB : 0; eR[i] = cp == NC + 1 ? OOB : 0;
        } else if (u < XPIECES + 16) {
            const int r = 8 * (u - XPIECES) + rr, h = r / NC, col = r % NC;
            voff[i] = (unsigned)(((col * H + h) * g.Cout + co0 + qsrc) * 2);
        }
    }
    const int xstep = 128 * g.Cin * 2, ystep = 128 * g.Cout * 2;            // bytes per step
    const int wc0 = (kbeg / H) % W;                     // column (within its image) of the split's first pixel
    auto stage_load = [&](int step, int buf, int wcs /* column of that step's first pixel */) {
        const unsigned selL = wcs == 0 ? OOB : 0u, selR = wcs + NC == W ? OOB : 0u;
#pragma unroll
        for (int i = 0; i < W9_NDMA; ++i) {
            const int u = wave + 8 * i;
            lptr_t dst = (lptr_t)(smem + buf * W9_STAGE + u * 1024);
            if (u < XPIECES) {
                const unsigned vo = voff[i] | (eL[i] & selL) | (eR[i] & selR);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xsrd, dst, 16, (int)vo, step * xstep, 0, 0);
            } else {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ysrd, dst, 16, (int)voff[i], step * ystep, 0, 0);
            }
        }
    };

    // ---- fragment addressing (loop invariant): lane (g4, L) supplies row 4 g4 + (L >> 2) of a 4 x 16 block, 8-byte piece L & 3
    const int g4 = lane >> 4, L = lane & 15;
    unsigned baseA[3], zabs[3], offB[4];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int cp = 1 + 4 * g4 + (L >> 2) + (d - 1);                          // plane row of the element this lane supplies (+16 for the second read at H = 4)
        baseA[d] = cp * 128 + ((cb ^ ((cp >> 1) & 3)) << 5) + (L & 3) * 8;
        zabs[d] = lds0 + W9_ZOFF + baseA[d];
    }
    const int clo = 4 * g4 + (L >> 2);                 // GENW: local column of the pixel this lane supplies (second read at H = 4: + 16)
    // ... and where it reads instead when that pixel's dw = -1 / +1 neighbour belongs to another image: a zero row, at the 8-byte piece it would have read
    const unsigned zlo0 = ZLO * 128 + (baseA[0] & 127), zlo2 = ZLO * 128 + (baseA[2] & 127);
    const unsigned zhi0 = ZHI * 128 + (baseA[0] & 127), zhi2 = ZHI * 128 + (baseA[2] & 127);
    const int rowl = kh * 64 + 4 * g4 + (L >> 2);
#pragma unroll
    for (int c = 0; c < 4; ++c) offB[c] = XROWS * 128 + rowl * 128 + ((c ^ ((rowl >> 1) & 3)) << 5) + (L & 3) * 8;
    *(u32x4*)(smem + W9_ZOFF + tid * 16) = (u32x4){0, 0, 0, 0};                   // 512 threads x 16 B (visible after the first barrier)

    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[t][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const unsigned offC = XROWS * 128 + w9_cs_offset(tid);

    int wcl = wc0;                                      // column of the next step to be loaded
    int wcc = wc0;                                      // GENW: column of the step being multiplied
#pragma unroll
    for (int p = 0; p < W9_NST - 1; ++p)
        if (p < nsteps) { stage_load(p, p, wcl); wcl += NC; if (wcl >= W) wcl -= W; }

    auto run = [&](auto khc) {
        constexpr int KH = decltype(khc)::value;
        int cur = 0;
        for (int step = 0; step < nsteps; ++step) {
            if (step + 1 < nsteps) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(W9_NDMA) : "memory");     // the next step may stay in flight
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const unsigned sb = lds0 + cur * W9_STAGE;
            unsigned sbA[3], sbAh[3], sbB[4];
#pragma unroll
            for (int d = 0; d < 3; ++d) { sbA[d] = sb + baseA[d]; sbAh[d] = sbA[d]; }
            if (GENW && W - wcc < NC) {
                // (uniform branch) this step crosses an image boundary at local column bq: the -1 tap of column bq and the +1 tap of column bq - 1 read zeros
                const int bq = W - wcc, chi = clo + (H == 4 ? 16 : 0);
                if (clo == bq) sbA[0] = sb + zlo0;
                if (clo == bq - 1) sbA[2] = sb + zlo2;
                if (chi == bq) sbAh[0] = sb + zhi0;
                if (chi == bq - 1) sbAh[2] = sb + zhi2;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) sbB[c] = sb + offB[c];
            s16x4 alo[W9_NSLOT], ahi[W9_NSLOT], blo[2][4], bhi[2][4];
            auto issue = [&](auto pc) {                               // the reads of stream position P
                constexpr int P = decltype(pc)::value;
                if constexpr (P == 0 || P == 10) {
                    constexpr int kb = P == 0 ? 0 : 1;
#pragma unroll
                    for (int c = 0; c < 4; ++c) { w9_tr(blo[kb][c], sbB[c], kb * 32 * 128); w9_tr(bhi[kb][c], sbB[c], kb * 32 * 128 + 16 * 128); }
                } else {
                    constexpr int m = P < 10 ? P - 1 : P - 2, kb = m / 9, tt = m % 9, dw = tt / 3, dh = tt % 3 - 1;
                    constexpr int pl = w9p_plane(H, KH, kb, dh, 0), ph = w9p_plane(H, KH, kb, dh, 1);
                    constexpr int il = pl >= 0 ? pl * PS * 128 : 0, ih = (ph >= 0 ? ph * PS * 128 : 0) + (H == 4 ? 16 * 128 : 0);
                    w9_tr(alo[m % W9_NSLOT], pl >= 0 ? sbA[dw] : zabs[dw], il);
                    w9_tr(ahi[m % W9_NSLOT], ph >= 0 ? sbAh[dw] : zabs[dw], ih);
                }
            };
            w9_for<0, 17>([&](auto nc) {
                constexpr int n = decltype(nc)::value, kk = n / 9, t = n % 9, dh = t % 3 - 1;
                if constexpr (n == W9_DMA_AT) {
                    // the buffer of step + 2 was last read in step - 1: free since this step's barrier
                    if (step + 2 < nsteps) { int nb = cur + 2; if (nb >= W9_NST) nb -= W9_NST; stage_load(step + 2, nb, wcl); wcl += NC; if (wcl >= W) wcl -= W; }
                }
                if constexpr (n == 0) w9_for<0, W9_TAB.upto[0]>(issue);                   // advance the read stream
                else w9_for<W9_TAB.upto[n > 0 ? n - 1 : 0] + 1, W9_TAB.upto[n]>(issue);
                w9_wait(W9_TAB.wait[n]);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (w9p_plane(H, KH, kk, dh, 0) >= 0 || w9p_plane(H, KH, kk, dh, 1) >= 0)      // an MFMA whose 32 pixels are all padding is not issued
                    w9_mfma_tap(acc[t], alo[n % W9_NSLOT], ahi[n % W9_NSLOT], blo[kk], bhi[kk]);
                __builtin_amdgcn_sched_barrier(0);
            });
            if (do_cs) w9_cs_step(cs, sb + offC);
            cur = (cur + 1 == W9_NST) ? 0 : cur + 1;
            if (GENW) { wcc += NC; if (wcc >= W) wcc -= W; }
        }
    };
    if (kh == 0) run(std::integral_constant<int, 0>{}); else run(std::integral_constant<int, 1>{});
    __syncthreads();                                   // every DMA has landed and every tile is dead: LDS is reused below
    W9P_PHASE(1);

    if (do_cs) w9_cs_store(g, smem, cs, split, co0, tid);
    W9P_PHASE(2);
    w9_store_tile(g, smem, acc, split, ci0, co0, cb, kh, lane);
#ifdef OCR_EXPERIMENTS
    W9P_PHASE(3);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    W9P_PHASE(4);
#endif
}
template <int H, bool GENW>
__global__ __launch_bounds__(512) void wgrad9p_kernel(W9Args g) { wgrad9p_body<H, GENW>(g, blockIdx.x); }

// TWO layers' workgroups in ONE grid: blocks [0, nblk_first) are the `first` job's, on wgrad9_kernel's body, the rest the `second` job's on
// the body <H, GENW> names (H = 16: wgrad9_kernel's body again) — gemm_tn3_kernel(j0, j1, nblk0)'s shape, both jobs as kernel arguments.
// A layer whose grid fills half the chip or less (conv2: 2 tiles x 64 splits = 128 workgroups of 16 steps on 256 CUs) goes FIRST, so
// its long, few workgroups start at once; the second layer's start on the CUs it leaves empty and follow on whichever CU frees up.
// Every workgroup runs exactly the code and the (split, tile) it has in a launch of its own: the slabs are the same words.
// (An overload of wgrad9p_kernel, not a new name: the profile summaries account the slab kernels by that symbol prefix.)
template <int H, bool GENW>
__global__ __launch_bounds__(512) void wgrad9p_kernel(W9Args first, W9Args second, int nblk_first) {
    const int b = blockIdx.x;
    if (b < nblk_first) wgrad9_body(first, b);
    else if constexpr (H == 16) wgrad9_body(second, b - nblk_first);
    else wgrad9p_body<H, GENW>(second, b - nblk_first);
}

// dw[i] += sum_s part[s][i];  dbias[co] += sum_s cs_part[s][co] — fixed summation order: deterministic.
// 256 threads = `rows` thread rows x (256 / rows) float4 columns, rows = S / 8 clamped to [1, 8]: every thread adds up to eight slabs
// (s = row, row + rows, ...) with all its loads in flight, then the rows meet in LDS.  (One load per thread — eight rows for any S —
// ran the S = 4 .. 16 layers at 2.8 TB/s; a plain loop over all slabs per column left conv2's S = 64 to a handful of CUs.)
__device__ __forceinline__ void w9_reduce_body(float* __restrict__ dw, const float* __restrict__ part, long n4, long slab4, int S, int rows,
                                               float* __restrict__ dbias, const float* __restrict__ cs_part, int Cout, int blk) {
    __shared__ f32x4 red[256];
    const int cols = 256 / rows;
    const int col = threadIdx.x % cols, row = threadIdx.x / cols;
    const long i = (long)blk * cols + col;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, t = a;
    if (i < n4) {
        f32x4 b = {0.f, 0.f, 0.f, 0.f}, c = b, d = b;
        const f32x4* p = (const f32x4*)part + i;
        // (round 5: the slabs are read exactly once — non-temporal loads keep them from displacing what the next kernels re-read from L2 — and
        //  the running gradient is fetched BEFORE the rows meet, not behind the barrier; same summation order, bit-identical results)
        if (row == 0) t = ((const f32x4*)dw)[i];
        int s = row;
        for (; s + 3 * rows < S; s += 4 * rows) {        // four slabs per round, the rounds independent of each other
            a += __builtin_nontemporal_load(p + (long)s * slab4);              b += __builtin_nontemporal_load(p + (long)(s + rows) * slab4);
            c += __builtin_nontemporal_load(p + (long)(s + 2 * rows) * slab4); d += __builtin_nontemporal_load(p + (long)(s + 3 * rows) * slab4);
        }
        for (; s < S; s += rows) a += __builtin_nontemporal_load(p + (long)s * slab4);
        a = (a + b) + (c + d);
    }
    red[row * cols + col] = a;
    __syncthreads();
    if (row == 0 && i < n4) {
        for (int r = 0; r < rows; ++r) t += red[r * cols + col];
        ((f32x4*)dw)[i] = t;
    }
    if (dbias != nullptr && blk == 0)
        for (int c = threadIdx.x; c < Cout; c += blockDim.x) {
            float t = dbias[c];
            for (int s = 0; s < S; ++s) t += cs_part[(long)s * Cout + c];
            dbias[c] = t;
        }
}
__global__ __launch_bounds__(256) void wgrad9_reduce_kernel(float* __restrict__ dw, const float* __restrict__ part, long n4, long slab4,
                                                            int S, int rows, float* __restrict__ dbias, const float* __restrict__ cs_part, int Cout) {
    w9_reduce_body(dw, part, n4, slab4, S, rows, dbias, cs_part, Cout, blockIdx.x);
}
// The reductions of SEVERAL layers in one launch (ocr_wgrad9_reduce_jobs): the per-layer reduce kernels are short (10 - 19 us, the
// smallest ones bound by their launch, not by their 19 MB) and each ends a dependent-kernel boundary; a backward pass that
// keeps every layer's slabs until its end pays for one launch instead of five.  Same per-element summation order as the
// per-layer kernel, hence bit-identical results.
struct W9ReduceJob {        // 64 bytes, mirrored by lstm_ctc_ocr_amd/engine.py (numpy structured dtype)
    float* dw; const float* part; float* dbias; const float* cs_part;
    long n4, slab4;
    int S, rows, Cout, block_start;
};
__global__ __launch_bounds__(256) void wgrad9_reduce_jobs_kernel(const W9ReduceJob* __restrict__ jobs, int njobs) {
    // the block's job = the last one whose block_start <= blockIdx.x, looked up by all threads at once (round 6: the serial scan was one dependent L2
    // round trip per job in front of every block; stream_ops.hip::pack_jobs_kernel)
    __shared__ int jsel[4];
    int j = 0;
    for (int k = threadIdx.x; k < njobs; k += 256)
        if (jobs[k].block_start <= (int)blockIdx.x) j = k;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) j = max(j, __shfl_xor(j, off));
    if ((threadIdx.x & 63) == 0) jsel[threadIdx.x >> 6] = j;
    __syncthreads();
    j = max(max(jsel[0], jsel[1]), max(jsel[2], jsel[3]));
    const W9ReduceJob jb = jobs[j];
    w9_reduce_body(jb.dw, jb.part, jb.n4, jb.slab4, jb.S, jb.rows, jb.dbias, jb.cs_part, jb.Cout, (int)blockIdx.x - jb.block_start);
}

struct W9Plan { int S, k_per_split, map, T_ci, T_co; size_t bytes; };

static bool w9_plan(int M, int W, int H, int Cin, int Cout, W9Plan* p) {
    if ((Cin & 63) || (Cout & 63) || (H != 2 && H != 4 && H != 8 && H != 16) || M < 512 || (M % H) || W * H < 32) return false;
    const int T_ci = Cin / 64, T_co = Cout / 64, T = T_ci * T_co;
    static int smax = -1;                       // A/B knob OCR_W9_SMAX: cap on the split count (partial slabs cost 2 x 147 KB x workgroups of HBM traffic)
    if (smax < 0) { const char* e = ocr_tune_env("OCR_W9_SMAX"); smax = e ? atoi(e) : 64; if (smax < 1) smax = 1; }
    int S = 1;
    while ((long)S * 2 * T <= 256 && S * 2 <= smax && M / (S * 2) >= 512) S *= 2;   // <= one workgroup per CU, >= four steps each
    p->S = S; p->T_ci = T_ci; p->T_co = T_co;
    p->k_per_split = ceil_div(ceil_div(M, S), 128) * 128;
    p->map = S >= 8 ? 1 : ((T % (8 / S)) == 0 ? 2 : 0);
    p->bytes = (size_t)S * ((size_t)9 * Cin * Cout + Cout) * sizeof(float);
    return true;
}

// Phase stamps of wgrad9p_kernel (experiments build only: W9P_PHASE; the product library stores the pointer and never reads it)
extern "C" int ocr_wgrad9_debug(void* dbg /* device int64[workgroups][8] or NULL */) {
    long long* q = (long long*)dbg;
    return hipMemcpyToSymbol(HIP_SYMBOL(w9_dbg), &q, sizeof(q)) == hipSuccess ? OCR_OK : OCR_ERR_MEMOPS;
}

extern "C" int ocr_conv3x3_wgrad_workspace_size(int Nb, int W, int H, int Cin, int Cout, size_t* bytes) {
    if (!bytes || Nb <= 0 || W <= 0 || H <= 0 || Cin <= 0 || Cout <= 0) return OCR_ERR_INVALID;
    W9Plan p;
    *bytes = w9_plan(Nb * W * H, W, H, Cin, Cout, &p) ? p.bytes : 0;
    return OCR_OK;
}

// Which slab kernel takes a covered shape: the decision wgrad9_try_dispatch launches by and ocr_conv3x3_wgrad_kernel_choice reports
// (gemm_tn.hip; the W9K_* codes are the first five of that query's).  -1: w9_plan refuses the shape.
enum { W9K_WGRAD9 = 0, W9K_P4 = 1, W9K_P8 = 2, W9K_P4_ZERO_ROW = 3, W9K_P8_ZERO_ROW = 4 };
static int w9_choose(int M, int W, int H, int Cin, int Cout, W9Plan* p) {
    if (!w9_plan(M, W, H, Cin, Cout, p)) return -1;
    // plane-layout kernel where it covers the shape (A/B knob OCR_W9_PLANES = 0: wgrad9_kernel everywhere)
    static int planes = -1;
    if (planes < 0) { const char* e = getenv("OCR_W9_PLANES"); planes = e ? atoi(e) : 1; }
    // whole-image steps (W % NC == 0) or, round 6, any W >= NC through the zero-row instances (GENW)
    static int genw = -1;                       // A/B knob OCR_W9P_GENW = 0: general widths stay on wgrad9_kernel; 2: the zero-row instances on whole-image shapes too (tests, timing)
    if (genw < 0) { const char* e = getenv("OCR_W9P_GENW"); genw = e ? atoi(e) : 1; }
    const bool whole = (H == 4 || H == 8) && W % (128 / H) == 0;
    const bool use_p = planes && (H == 4 || H == 8) && (whole || (genw && W >= 128 / H)) && M % 128 == 0 &&
                       (long)M * (Cin > Cout ? Cin : Cout) * 2 < 0x7fffffffL;
    if (!use_p) return W9K_WGRAD9;              // (H = 2 and H = 16 always: wgrad9p has no instance for them)
    if (!whole || (genw == 2 && W >= 128 / H)) return H == 4 ? W9K_P4_ZERO_ROW : W9K_P8_ZERO_ROW;
    return H == 4 ? W9K_P4 : W9K_P8;
}
int wgrad9_choice(int Nb, int W, int H, int Cin, int Cout, int* S) {
    W9Plan p;
    const int k = w9_choose(Nb * W * H, W, H, Cin, Cout, &p);
    if (k >= 0) *S = p.S;
    return k;
}

// (function-pointer constants: wgrad9p_kernel<H, GENW> names two overloads, the single-job and the paired kernel)
typedef void (*W9Kernel)(W9Args);
typedef void (*W9PairKernel)(W9Args, W9Args, int);
template <int H, bool GENW> constexpr W9Kernel W9P_SINGLE = wgrad9p_kernel<H, GENW>;
template <int H, bool GENW> constexpr W9PairKernel W9P_PAIR = wgrad9p_kernel<H, GENW>;

template <auto KERNEL>
static int w9_launch(const W9Args& g, int grid, hipStream_t stream) {
    if (ocr_allow_lds<KERNEL>(W9_LDS) != hipSuccess) return OCR_ERR_EXEC;
    KERNEL<<<grid, 512, W9_LDS, stream>>>(g);
    return OCR_OK;
}
template <auto KERNEL>
static int w9_launch_pair(const W9Args& first, int grid_first, const W9Args& second, int grid_second, hipStream_t stream) {
    if (ocr_allow_lds<KERNEL>(W9_LDS) != hipSuccess) return OCR_ERR_EXEC;
    KERNEL<<<grid_first + grid_second, 512, W9_LDS, stream>>>(first, second, grid_first);
    return OCR_OK;
}

// plan + kernel arguments of one layer, as every launch form sets them up; -1: shape not covered or workspace too small
static int w9_setup(const void* x, const void* dy, float* dbias, int Nb, int W, int H, int Cin, int Cout, void* workspace, size_t ws_bytes,
                    W9Plan* p, W9Args* g) {
    const int M = Nb * W * H;
    if (!workspace) return -1;
    const int kern = w9_choose(M, W, H, Cin, Cout, p);
    if (kern < 0 || ws_bytes < p->bytes) return -1;
    *g = W9Args{};
    g->X = (const bf16_t*)x; g->dY = (const bf16_t*)dy; g->M = M; g->Cin = Cin; g->Cout = Cout; g->cW = W; g->cH = H;
    g->k_per_split = p->k_per_split; g->S = p->S; g->T_ci = p->T_ci; g->T_co = p->T_co; g->map = p->map;
    g->part = (float*)workspace;
    g->cs_part = dbias ? g->part + (size_t)p->S * 9 * Cin * Cout : nullptr;
    return kern;
}
// the reduction that follows a layer's slab kernel: its job record and block count
static W9ReduceJob w9_reduce_job(const W9Args& g, float* dw, float* dbias, int* blocks) {
    const long n4 = (long)9 * g.Cin * g.Cout / 4;
    int rows = g.S / 8;
    rows = rows < 1 ? 1 : (rows > 8 ? 8 : rows);
    while (rows & (rows - 1)) rows &= rows - 1;                       // power of two
    const int cols = 256 / rows;
    *blocks = (int)((n4 + cols - 1) / cols);
    return W9ReduceJob{dw, g.part, dbias, g.cs_part, n4, n4, g.S, rows, g.Cout, 0};
}

// -1: shape not covered or workspace too small (caller falls back to the atomics kernels)
int wgrad9_try_dispatch(const void* x, const void* dy, float* dw, float* dbias, int Nb, int W, int H, int Cin, int Cout,
                        void* workspace, size_t ws_bytes, hipStream_t stream, void* defer_job, int* defer_blocks) {
    W9Plan p;
    W9Args g;
    const int kern = w9_setup(x, dy, dbias, Nb, W, H, Cin, Cout, workspace, ws_bytes, &p, &g);
    if (kern < 0) return -1;
    const int grid = p.S * p.T_ci * p.T_co;
    int rc;
    switch (kern) {
        case W9K_P4: rc = w9_launch<W9P_SINGLE<4, false>>(g, grid, stream); break;
        case W9K_P8: rc = w9_launch<W9P_SINGLE<8, false>>(g, grid, stream); break;
        case W9K_P4_ZERO_ROW: rc = w9_launch<W9P_SINGLE<4, true>>(g, grid, stream); break;
        case W9K_P8_ZERO_ROW: rc = w9_launch<W9P_SINGLE<8, true>>(g, grid, stream); break;
        default: rc = w9_launch<wgrad9_kernel>(g, grid, stream); break;
    }
    if (rc != OCR_OK) return rc;
    OCR_CHECK_LAUNCH();
    int blocks;
    const W9ReduceJob jb = w9_reduce_job(g, dw, dbias, &blocks);
    if (defer_job != nullptr) {                                       // the caller runs this reduction later, with others, in one launch
        *(W9ReduceJob*)defer_job = jb;
        *defer_blocks = blocks;
        return OCR_OK;
    }
    wgrad9_reduce_kernel<<<blocks, 256, 0, stream>>>(dw, g.part, jb.n4, jb.slab4, jb.S, jb.rows, dbias, g.cs_part, Cout);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}

// ---- two layers in one launch -----------------------------------------------------------------------------------------------------
// THE pairing policy, stated once (ocr_conv3x3_wgrad_pair_supported and the launch both ask here): both shapes take a slab kernel, the
// first one wgrad9_kernel (the paired instances are wgrad9 + {wgrad9, the four wgrad9p bodies}), and the first job's grid leaves at least
// half the chip empty — only then is there room for the second job's workgroups beside it.
bool wgrad9_pair_ok(int Nb0, int W0, int H0, int Cin0, int Cout0, int Nb1, int W1, int H1, int Cin1, int Cout1) {
    W9Plan p0, p1;
    if (w9_choose(Nb0 * W0 * H0, W0, H0, Cin0, Cout0, &p0) != W9K_WGRAD9) return false;
    if (w9_choose(Nb1 * W1 * H1, W1, H1, Cin1, Cout1, &p1) < 0) return false;
    return 2 * p0.S * p0.T_ci * p0.T_co <= ocr_cu_count();
}

// -1: the pair is not supported (policy above) or a workspace is too small: nothing was launched
int wgrad9_try_dispatch_pair(const void* const x[2], const void* const dy[2], float* const dw[2], float* const dbias[2], const int shape0[5],
                             const int shape1[5], void* const workspace[2], const size_t ws_bytes[2], hipStream_t stream, void* const job[2],
                             int* const job_blocks[2]) {
    if (!wgrad9_pair_ok(shape0[0], shape0[1], shape0[2], shape0[3], shape0[4], shape1[0], shape1[1], shape1[2], shape1[3], shape1[4])) return -1;
    W9Plan p0, p1;
    W9Args g0, g1;
    const int k0 = w9_setup(x[0], dy[0], dbias[0], shape0[0], shape0[1], shape0[2], shape0[3], shape0[4], workspace[0], ws_bytes[0], &p0, &g0);
    const int k1 = w9_setup(x[1], dy[1], dbias[1], shape1[0], shape1[1], shape1[2], shape1[3], shape1[4], workspace[1], ws_bytes[1], &p1, &g1);
    if (k0 != W9K_WGRAD9 || k1 < 0) return -1;
    // Each job keeps the grid, the split count and the workgroup map of its own launch.  The maps place a job's workgroups on the eight XCDs by
    // (index within the job) & 7 while the hardware deals by blockIdx & 7: where grid0 is no multiple of 8 the second job's map is rotated
    // against the XCDs — its splits lose their L2 locality, the (split, tile) every workgroup computes and stores stays the same.
    const int grid0 = p0.S * p0.T_ci * p0.T_co, grid1 = p1.S * p1.T_ci * p1.T_co;
    int rc;
    switch (k1) {
        case W9K_P4: rc = w9_launch_pair<W9P_PAIR<4, false>>(g0, grid0, g1, grid1, stream); break;
        case W9K_P8: rc = w9_launch_pair<W9P_PAIR<8, false>>(g0, grid0, g1, grid1, stream); break;
        case W9K_P4_ZERO_ROW: rc = w9_launch_pair<W9P_PAIR<4, true>>(g0, grid0, g1, grid1, stream); break;
        case W9K_P8_ZERO_ROW: rc = w9_launch_pair<W9P_PAIR<8, true>>(g0, grid0, g1, grid1, stream); break;
        default: rc = w9_launch_pair<W9P_PAIR<16, false>>(g0, grid0, g1, grid1, stream); break;
    }
    if (rc != OCR_OK) return rc;
    OCR_CHECK_LAUNCH();
    *(W9ReduceJob*)job[0] = w9_reduce_job(g0, dw[0], dbias[0], job_blocks[0]);
    *(W9ReduceJob*)job[1] = w9_reduce_job(g1, dw[1], dbias[1], job_blocks[1]);
    return OCR_OK;
}

extern "C" int ocr_wgrad9_reduce_jobs(const void* jobs, int njobs, int total_blocks, void* stream) {
    static_assert(sizeof(W9ReduceJob) == 64, "W9ReduceJob is mirrored by engine.py");
    if (!jobs || njobs <= 0 || total_blocks <= 0) return OCR_ERR_INVALID;
    wgrad9_reduce_jobs_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>((const W9ReduceJob*)jobs, njobs);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
