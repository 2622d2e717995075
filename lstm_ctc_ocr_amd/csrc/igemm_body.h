// The large-tile bf16 MFMA engine's workgroup as a device function (igemm.hip has the design notes): arguments, the workgroup's index within
// ITS OWN grid, the base of its dynamic LDS and a 64-byte page of zeros.  igemm.hip's igemm_kernel runs it as a launch of its own;
// gemm_tn3.hip's gemm_tn3_nt_kernel runs the plain-mode eight-wave instance on the CUs a plain weight-gradient launch leaves idle.
#pragma once
#include "common.h"

enum { IG_BIAS = 1, IG_RELU = 2, IG_OUT_F32 = 4, IG_MASK = 16, IG_ROWSWAP = 32 };

struct IgArgs {
    const bf16_t* P; const bf16_t* Q;
    long ldp, ldq;
    int M, N, K;              // K % 64 == 0
    int grp, skip;            // plain mode row groups
    int cW, cH, cC;           // conv mode geometry, cC % 64 == 0
    void* out; long ldo;
    const float* bias; const bf16_t* mask; long ldmask;
    int flags, swap_inner, swap_outer;
};

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// dynamic LDS of an instance: STAGES x (P tile | Q tile)
template <int BN, int STAGES, int NW>
constexpr int ig_lds_bytes() { return STAGES * (32 * NW * 128 + BN * 128); }

template <int BN, int MODE /*0 plain, 1 conv3x3*/, int STAGES /*2 or 3 LDS stages*/, int NW /*waves: 8 (256-row tiles) or 4 (128-row tiles, two workgroups per CU)*/>
__device__ __forceinline__ void ig_body(const IgArgs& g, const int bid, unsigned char* smem, const bf16_t* zero) {
    constexpr int BM = 32 * NW, BK = 64;
    constexpr int WAVES_N = BN / 64, WAVES_M = NW / WAVES_N;
    constexpr int WM = BM / WAVES_M;               // 128 / 64 / 32
    constexpr int FM = WM / 16, FN = 4;
    constexpr int PB = BM * BK * 2, QB = BN * BK * 2, STAGE = PB + QB;
    constexpr int QI = BN / (8 * NW);              // Q DMA instructions per wave per stage (P: always 4)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;

    // XCD-aware tile order: consecutive logical tiles live on one XCD
    const int mtiles = (g.M + BM - 1) / BM, ntiles = (g.N + BN - 1) / BN;
    const int nblk = mtiles * ntiles;
    int L = bid;
    if ((nblk & 7) == 0) L = (L & 7) * (nblk >> 3) + (L >> 3);
    const int m0 = (L / ntiles) * BM, n0 = (L % ntiles) * BN;

    // ---- per-thread DMA source rows (fixed over the K loop); LDS chunk position lane&7 holds source chunk (lane&7)^(lane>>3)
    const int rsub = lane >> 3;
    const int csrc = ((lane & 7) ^ rsub) * 8;       // element offset of the 16-B source chunk inside the 64-wide K tile
    const bf16_t* prow[4];
    int pw[4], ph[4];
    bool pok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int m = m0 + (wave * 4 + j) * 8 + rsub;
        pok[j] = m < g.M;
        int mm = pok[j] ? m : 0;
        if (MODE == 0) {
            long phys = (long)mm + (g.grp > 0 ? (long)(mm / g.grp) * g.skip : 0);
            prow[j] = g.P + phys * g.ldp + csrc;
            pw[j] = ph[j] = 0;
        } else {
            ph[j] = mm % g.cH;
            pw[j] = (mm / g.cH) % g.cW;
            prow[j] = g.P + (long)mm * g.cC + csrc;
        }
    }
    const bf16_t* qrow[QI];
#pragma unroll
    for (int j = 0; j < QI; ++j) {
        int n = n0 + (wave * QI + j) * 8 + rsub;
        qrow[j] = (n < g.N) ? g.Q + (long)n * g.ldq + csrc : nullptr;
    }

    auto stage_load = [&](int k0, int buf) {
        unsigned char* sp = smem + buf * STAGE;
        long shift = k0;
        int dw = 0, dh = 0;
        if (MODE == 1) {
            int tap = k0 / g.cC;                    // uniform: cC % 64 == 0 keeps a K tile inside one tap
            dw = tap / 3 - 1; dh = tap % 3 - 1;
            shift = ((long)dw * g.cH + dh) * g.cC + (k0 - tap * g.cC);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool ok = pok[j];
            if (MODE == 1) ok = ok && (unsigned)(pw[j] + dw) < (unsigned)g.cW && (unsigned)(ph[j] + dh) < (unsigned)g.cH;
            const bf16_t* src = ok ? prow[j] + shift : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sp + (wave * 4 + j) * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < QI; ++j) {
            const bf16_t* src = qrow[j] ? qrow[j] + k0 : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sp + PB + (wave * QI + j) * 1024), 16, 0, 0);
        }
    };

    f32x4 acc[FN][FM];
#pragma unroll
    for (int a = 0; a < FN; ++a)
#pragma unroll
        for (int b = 0; b < FM; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // fragment read offsets: row (lane&15) of a 16-row block, 16-B chunk (kk*4 + lane>>4) ^ (row & 7)
    const int frow = lane & 15, fq = lane >> 4, fx = lane & 7;
    const int ntk = g.K / BK;
    constexpr int NI = 4 + QI;        // DMA instructions one wave issues per stage
    // All fragment reads of a K tile are issued back to back as inline asm (the compiler neither counts nor waits for them),
    // then one counted wait per K-half: the first half's FN + FM fragments were issued first and LDS returns in order.
    // (hipcc's own schedule interleaved small read groups with the MFMAs and drained lgkmcnt(0) several times per tile.)
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const unsigned qoff = PB + (wn * 64 + frow) * 128 + ((fq ^ fx) << 4);     // ^ 64 for the second K-half; + a * 2048
    const unsigned poff = (wm * WM + frow) * 128 + ((fq ^ fx) << 4);          // + b * 2048
    auto compute = [&](int buf) {
        const unsigned base = lds0 + buf * STAGE;
        u32x4 af[2][FN], bfr[2][FM];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
            for (int a = 0; a < FN; ++a)
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[kk][a]) : "v"(base + (qoff ^ (kk * 64))), "n"(a * 2048));
#pragma unroll
            for (int b = 0; b < FM; ++b)
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bfr[kk][b]) : "v"(base + (poff ^ (kk * 64))), "n"(b * 2048));
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (kk == 0) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(FN + FM) : "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int a = 0; a < FN; ++a)
#pragma unroll
                for (int b = 0; b < FM; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[kk][a]),
                                                                        __builtin_bit_cast(bf16x8, bfr[kk][b]), acc[a][b], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if (STAGES == 2) {
        stage_load(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int t = 0; t < ntk; ++t) {
            const int cur = t & 1;
            if (t + 1 < ntk) stage_load((t + 1) * BK, cur ^ 1);
            compute(cur);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // next stage has landed (this wave's DMA pieces)
            __syncthreads();                                     // everyone's pieces landed, everyone done reading `cur`
        }
    } else {
        // three stages, two K tiles in flight: the wait at the top of step t only retires stage t (counted vmcnt leaves the
        // NI DMA instructions of stage t+1 outstanding), and the barrier is a RAW s_barrier — __syncthreads() would drain
        // the DMA queue (an LDS-DMA is a pending LDS write on the VM counter).  The same barrier orders "everyone finished
        // reading stage t-1" before stage t+2 is streamed into that buffer.
        stage_load(0, 0);
        if (ntk > 1) stage_load(BK, 1);
        int cur = 0;
        for (int t = 0; t < ntk; ++t) {
            if (t + 1 < ntk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (t + 2 < ntk) { int nb = cur + 2; if (nb >= 3) nb -= 3; stage_load((t + 2) * BK, nb); }
            compute(cur);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's fragment reads of `cur` are complete
            cur = (cur == 2) ? 0 : cur + 1;
        }
    }

    // ---- epilogue: lane owns n = nb + (lane>>4)*4 .. +3 at m = mb + (lane&15).  Loop order m-block outer / n-fragment inner:
    // the FN stores that complete one 128-byte run of a pixel row are issued back to back (with n outer the same lines
    // were revisited FM stores apart and reached HBM as partial-line writes — WRITE_SIZE 2.5x the output bytes).
    const int flags = g.flags;
    f32x4 bv[FN];
#pragma unroll
    for (int a = 0; a < FN; ++a) {
        const int n = n0 + wn * 64 + a * 16 + (lane >> 4) * 4;
        bv[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if ((flags & IG_BIAS) && n < g.N) bv[a] = *(const f32x4*)(g.bias + n);
    }
#pragma unroll
    for (int b = 0; b < FM; ++b) {
        const int m = m0 + wm * WM + b * 16 + (lane & 15);
        if (m >= g.M) continue;
        long orow = m;
        if (flags & IG_ROWSWAP) orow = (long)(m % g.swap_inner) * g.swap_outer + m / g.swap_inner;
#pragma unroll
        for (int a = 0; a < FN; ++a) {
            const int n = n0 + wn * 64 + a * 16 + (lane >> 4) * 4;
            if (n >= g.N) continue;
            f32x4 v = acc[a][b] + bv[a];
            if (flags & IG_RELU) {
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
            if (flags & IG_MASK) {
                u32x2 mk = *(const u32x2*)(g.mask + (long)m * g.ldmask + n);
                if (!(bf_lo(mk.x) > 0.f)) v.x = 0.f;
                if (!(bf_hi(mk.x) > 0.f)) v.y = 0.f;
                if (!(bf_lo(mk.y) > 0.f)) v.z = 0.f;
                if (!(bf_hi(mk.y) > 0.f)) v.w = 0.f;
            }
            if (flags & IG_OUT_F32) {
                *(f32x4*)((float*)g.out + orow * g.ldo + n) = v;
            } else {
                u32x2 pk;
                pk.x = pack_bf2(v.x, v.y);
                pk.y = pack_bf2(v.z, v.w);
                *(u32x2*)((bf16_t*)g.out + orow * g.ldo + n) = pk;
            }
        }
    }
}

// Whether the large-tile engine takes a GEMM at all (ig_try_dispatch's first test; the paired launch's policy asks the same).
static inline bool ig_covers(int M, int N, int K, int flags, int mode, int cC) {
    if ((K & 63) || (N & 3) || M < 1024) return false;
    if (mode == 1 && (cC & 63)) return false;
    return !(flags & ~(IG_BIAS | IG_RELU | IG_OUT_F32 | IG_MASK | IG_ROWSWAP));       // atomics / accumulate: old kernel
}
