// Edit distance on the device for gfx950: Levenshtein distance (unit costs for insert, delete, substitute) between every string of a set A and
// every string of a set B per sample, the four sums a character error rate needs, and minimum-Bayes-risk selection over an n-best list's
// K x K distances.  Everything is integer or a fixed-order fp32 sum: the results are fully determined.  No atomics, no communication between
// workgroups, no spin; the waves of a workgroup do not communicate either (no barrier in the distance kernel).
//
// The recursion.  Row i of the table (D[i][j] = distance of A's first i characters to B's first j) from row i - 1:
//     t[j] = min(D[i-1][j] + 1, D[i-1][j-1] + (a_i != b_j)),  t[0] = i          what comes from above and from the diagonal, lane-local
//     D[i][j] = j + min over k <= j of (t[k] - k)                                the insertions from the left, as ONE prefix-min scan
// so the dependency inside a row is a scan across lanes and not a serial chain.  Lanes hold the columns (column j = sl * CPL + c of a segment's
// lane sl), the kernel iterates over the characters of A.  Columns beyond B's length compute values nobody reads: a column depends on the
// columns at and left of it only.
//
//   edit_distance_kernel   a wave per FOUR consecutive pairs (n, i, j), j fastest.  It reads the eight raw lengths and takes one of two routes,
//                          the choice wave-uniform (one __ballot):
//                            short  every string of the four pairs has a raw length of at most 15: each pair gets a 16-lane segment (column per
//                                   lane, columns 0 .. 15), the four tables advance together, the row loop runs to the longest A of the four
//                                   and masks the rest; shifts and the scan are DPP row shifts (a row IS a segment).
//                            long   the four pairs one after the other on all 64 lanes: one column per lane for a B of up to 63 characters, four
//                                   per lane up to 255; the shift by one is a DPP wave shift, the scan's larger steps are __shfl_up.
//                          The `ignore` class is dropped while loading: ballot + prefix popcount compact a string into the wave's own LDS copy
//                          (512 ints per wave).  A "no string" (raw length < 0 or above the pitch, or more than 255 characters counted)
//                          makes every pair it is in -1; its count is -1.
//   edit_stats_kernel      one workgroup: {sum of dist, sum of ref_count, pairs with dist == 0, pairs} over the pairs with dist >= 0.
//   mbr_select_kernel      one workgroup per sample, thread i the candidate i: the weights exp(c_min - c_j) once into LDS, then every thread its
//                          own two K-term sums in ascending j; thread 0 takes the arg-min under (risk, cost, index).
// Every loop bound and every branch around a cross-lane operation is wave-uniform: the bounds are taken from ballots, or made scalar with
// readfirstlane from values every lane computed alike.  No address at or beyond a string's start + pitch is read: a length is clamped to the pitch
// (such a string is "no string" and none of it is read) and the load loops run to the clamped length.
#include "ctc_common.h"
#include <math.h>

constexpr int ED_MAX_LEN = 255;                 // counted characters of a string
constexpr int ED_SHORT = 15;                    // raw length up to which a pair fits a 16-lane segment
constexpr int ED_NT = 256, ED_NW = ED_NT / 64;
constexpr int ED_GROUP = 4;                     // pairs of a wave
constexpr int ED_FAR = 1 << 20;                 // above every t[k] - k
constexpr long long ED_MAX_PAIRS = 1ll << 30;
constexpr int ED_STATS_NT = 1024;
constexpr int MBR_MAX_K = 128;

struct EdSet {
    const int* s;
    const int* len;
    long ld, sn;
    int K;
};
struct EdString {
    const int* at;
    int raw;                                    // the raw length; 0 when !ok
    bool ok;
};
__device__ __forceinline__ long ed_len_index(const EdSet& S, int n, int i) { return (S.sn ? (long)n * S.K : 0L) + i; }
__device__ __forceinline__ EdString ed_string(const EdSet& S, int n, int i) {
    EdString r;
    r.at = S.s + (long)n * S.sn + (long)i * S.ld;
    const int len = S.len[ed_len_index(S, n, i)];
    r.ok = len >= 0 && (long)len <= S.ld;
    r.raw = r.ok ? len : 0;
    return r;
}
// the wave's own LDS traffic: orders a lane's stores before the other lanes' loads (and the loads before the next stores)
__device__ __forceinline__ void ed_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// lane sl of a W-lane segment takes v of lane sl - D, `fill` where there is none.  W == 16: a DPP row shift (a row is a segment); W == 64: the
// DPP wave shift for D == 1, __shfl_up else.
template <int W, int D>
__device__ __forceinline__ int ed_shr(int v, int fill, int lane) {
    if constexpr (W == 16) return __builtin_amdgcn_update_dpp(fill, v, 0x110 + D, 0xf, 0xf, false);           // row_shr:D
    else if constexpr (D == 1) return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false);           // wave_shr:1
    else {
        const int o = __shfl_up(v, D, 64);
        return lane >= D ? o : fill;
    }
}
template <int W>
__device__ __forceinline__ int ed_scan_min(int s, int lane) {
    s = min(s, ed_shr<W, 1>(s, ED_FAR, lane));
    s = min(s, ed_shr<W, 2>(s, ED_FAR, lane));
    s = min(s, ed_shr<W, 4>(s, ED_FAR, lane));
    s = min(s, ed_shr<W, 8>(s, ED_FAR, lane));
    if constexpr (W == 64) {
        s = min(s, ed_shr<W, 16>(s, ED_FAR, lane));
        s = min(s, ed_shr<W, 32>(s, ED_FAR, lane));
    }
    return s;
}

// The table of one pair per W-lane segment: sa = the segment's A in LDS, La its length, `rows` the wave-uniform number of rows to run (the
// largest La of the wave's segments; rows beyond La leave the segment's table as it is), bch = B's character at this lane's columns (column
// j = sl * CPL + c holds b_j, 1 <= j <= Lb; anything else elsewhere), sl = the lane within the segment (the lane itself when W == 64).
// -> D[La][Lb] in every lane of the segment.
template <int CPL, int W>
__device__ __forceinline__ int ed_rows(const int* sa, int La, int rows, const int (&bch)[CPL], int Lb, int sl, int lane) {
    int prev[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) prev[c] = sl * CPL + c;                 // row 0
    for (int i = 1; i <= rows; ++i) {
        const int ai = sa[i - 1];
        const int left = ed_shr<W, 1>(prev[CPL - 1], 0, W == 64 ? lane : sl);      // D[i-1][j-1] of this lane's first column
        int u[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int j = sl * CPL + c;
            const int diag = c ? prev[c ? c - 1 : 0] : left;
            int t = min(prev[c] + 1, diag + (ai != bch[c] ? 1 : 0));
            if (j == 0) t = i;
            u[c] = t - j;
        }
#pragma unroll
        for (int c = 1; c < CPL; ++c) u[c] = min(u[c], u[c - 1]);
        const int incl = ed_scan_min<W>(u[CPL - 1], W == 64 ? lane : sl);
        const int excl = ed_shr<W, 1>(incl, ED_FAR, W == 64 ? lane : sl);  // the lanes to the left
        const bool live = i <= La;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int d = sl * CPL + c + min(u[c], excl);
            prev[c] = live ? d : prev[c];
        }
    }
    int pick = prev[0];
#pragma unroll
    for (int c = 1; c < CPL; ++c) pick = (Lb % CPL == c) ? prev[c] : pick;
    return __shfl(pick, (lane - sl) + Lb / CPL, 64);
}

// A string by the whole wave: its characters other than `ignore` into dst[0 .. 255), -> their number, -1 above 255.  raw is wave-uniform.
__device__ __forceinline__ int ed_pack_wave(const int* __restrict__ src, int raw, int ignore, int* dst, int lane) {
    int cnt = 0;
    for (int off = 0; off < raw; off += 64) {
        const int at = off + lane;
        const int ch = at < raw ? src[at] : 0;
        const bool keep = at < raw && (ignore < 0 || ch != ignore);
        const unsigned long long bal = __ballot(keep);
        const int pos = cnt + __popcll(bal & ((1ull << lane) - 1));
        if (keep && pos < ED_MAX_LEN) dst[pos] = ch;
        cnt += __popcll(bal);
        if (cnt > ED_MAX_LEN) break;                                      // (uniform: cnt comes from the ballot)
    }
    return cnt > ED_MAX_LEN ? -1 : cnt;
}
// A string of at most 15 raw characters by its own 16-lane segment: into dst[0 .. 15), -> their number
__device__ __forceinline__ int ed_pack_segment(const int* __restrict__ src, int raw, int ignore, int* dst, int sl, int seg) {
    const int ch = sl < raw ? src[sl] : 0;
    const bool keep = sl < raw && (ignore < 0 || ch != ignore);
    const unsigned bits = (unsigned)(__ballot(keep) >> (seg * 16)) & 0xffffu;
    if (keep) dst[__popc(bits & ((1u << sl) - 1))] = ch;
    return __popc(bits);
}
__device__ __forceinline__ void ed_store(const EdSet& A, const EdSet& B, int p, int n, int i, int j, int d, int ca, int cb, int* __restrict__ dist,
                                         int* __restrict__ a_count, int* __restrict__ b_count) {
    dist[p] = (ca >= 0 && cb >= 0) ? d : -1;
    if (a_count && j == 0 && (A.sn || n == 0)) a_count[ed_len_index(A, n, i)] = ca;          // each count by one pair only
    if (b_count && i == 0 && (B.sn || n == 0)) b_count[ed_len_index(B, n, j)] = cb;
}

__global__ __launch_bounds__(ED_NT) void edit_distance_kernel(EdSet A, EdSet B, int total, int ignore, int* __restrict__ dist,
                                                              int* __restrict__ a_count, int* __restrict__ b_count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sl = lane & 15, seg = lane >> 4;
    __shared__ int s_str[ED_NW][2][256];
    int* sa = s_str[wave][0];
    int* sb = s_str[wave][1];
    const long first = ((long)blockIdx.x * ED_NW + wave) * ED_GROUP;
    if (first >= total) return;                                           // (the whole wave)
    const int KK = A.K * B.K;

    // this lane's segment's pair
    const int p = (int)first + seg;
    const bool have = p < total;
    int n = 0, i = 0, j = 0;
    EdString a = {A.s, 0, false}, b = {B.s, 0, false};
    if (have) {
        n = p / KK;
        const int r = p - n * KK;
        i = r / B.K;
        j = r - i * B.K;
        a = ed_string(A, n, i);
        b = ed_string(B, n, j);
    }
    if (__ballot(a.raw > ED_SHORT || b.raw > ED_SHORT) == 0) {
        // ---- short: four tables at once, a segment each
        const int La = ed_pack_segment(a.at, a.raw, ignore, sa + seg * 16, sl, seg);
        const int Lb = ed_pack_segment(b.at, b.raw, ignore, sb + seg * 16, sl, seg);
        ed_wave_sync();
        const int bch[1] = {(sl >= 1 && sl <= Lb) ? sb[seg * 16 + sl - 1] : -1};
        int rows = max(max(__shfl(La, 0, 64), __shfl(La, 16, 64)), max(__shfl(La, 32, 64), __shfl(La, 48, 64)));
        rows = __builtin_amdgcn_readfirstlane(rows);
        const int d = ed_rows<1, 16>(sa + seg * 16, La, rows, bch, Lb, sl, lane);
        if (have && sl == 0) ed_store(A, B, p, n, i, j, d, a.ok ? La : -1, b.ok ? Lb : -1, dist, a_count, b_count);
        return;
    }
    // ---- long: the pairs one after the other on the whole wave
    for (int q = 0; q < ED_GROUP; ++q) {
        const int pq = (int)first + q;
        if (pq >= total) break;                                           // (uniform)
        const int nq = pq / KK, rq = pq - nq * KK, iq = rq / B.K, jq = rq - iq * B.K;
        const EdString aq = ed_string(A, nq, iq), bq = ed_string(B, nq, jq);
        const int rawA = __builtin_amdgcn_readfirstlane(aq.raw), rawB = __builtin_amdgcn_readfirstlane(bq.raw);
        const bool okA = __builtin_amdgcn_readfirstlane((int)aq.ok) != 0, okB = __builtin_amdgcn_readfirstlane((int)bq.ok) != 0;
        ed_wave_sync();                                                   // the last pair's reads of sa / sb are done
        int La = ed_pack_wave(aq.at, rawA, ignore, sa, lane);
        int Lb = ed_pack_wave(bq.at, rawB, ignore, sb, lane);
        La = okA ? La : -1;
        Lb = okB ? Lb : -1;
        ed_wave_sync();
        int d = -1;
        if (La >= 0 && Lb >= 0) {                                         // (uniform)
            if (Lb <= 63) {
                const int bch[1] = {(lane >= 1 && lane <= Lb) ? sb[lane - 1] : -1};
                d = ed_rows<1, 64>(sa, La, La, bch, Lb, lane, lane);
            } else {
                int bch[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int col = lane * 4 + c;
                    bch[c] = (col >= 1 && col <= Lb) ? sb[col - 1] : -1;
                }
                d = ed_rows<4, 64>(sa, La, La, bch, Lb, lane, lane);
            }
        }
        if (lane == 0) ed_store(A, B, pq, nq, iq, jq, d, La, Lb, dist, a_count, b_count);
    }
}

__device__ __forceinline__ long long ed_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)((unsigned long long)v >> 32), o, 64);
        v += (long long)(((unsigned long long)hi << 32) | lo);
    }
    return v;
}
__global__ __launch_bounds__(ED_STATS_NT) void edit_stats_kernel(const int* __restrict__ dist, const int* __restrict__ ref_count, long M,
                                                                 long long* __restrict__ stats) {
    constexpr int NW = ED_STATS_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long v[4] = {0, 0, 0, 0};
    for (long m = tid; m < M; m += ED_STATS_NT) {
        const int d = dist[m];
        if (d >= 0) { v[0] += d; v[1] += ref_count[m]; v[2] += d == 0; v[3] += 1; }
    }
    __shared__ long long s_part[NW][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long s = ed_wave_sum(v[k]);
        if (lane == 0) s_part[wave][k] = s;
    }
    __syncthreads();
    if (tid < 4) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) s += s_part[w][tid];
        stats[tid] = s;
    }
}

__global__ __launch_bounds__(MBR_MAX_K) void mbr_select_kernel(const int* __restrict__ dist, const float* __restrict__ costs, int K,
                                                               float* __restrict__ risk, int* __restrict__ best, float* __restrict__ best_risk) {
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int* D = dist + (size_t)n * K * K;
    __shared__ float s_w[MBR_MAX_K], s_cost[MBR_MAX_K], s_risk[MBR_MAX_K], s_min[MBR_MAX_K / 64];
    __shared__ int s_ok[MBR_MAX_K];
    float c = INFINITY;
    bool ok = false;
    if (t < K) {
        c = costs[(size_t)n * K + t];
        ok = fabsf(c) < INFINITY && D[(size_t)t * K + t] >= 0;           // (NaN compares false)
    }
    float m = ok ? c : INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
    if (lane == 0) s_min[wave] = m;
    __syncthreads();
    const float c_min = fminf(s_min[0], s_min[1]);
    s_w[t] = ok ? expf(__fsub_rn(c_min, c)) : 0.f;
    s_ok[t] = ok;
    s_cost[t] = c;
    __syncthreads();
    float r = INFINITY;
    if (ok) {
        float Z = 0.f, acc = 0.f;
        for (int j = 0; j < K; ++j) {                                     // ascending j, one rounding per operation: the same sums in every launch
            if (!s_ok[j]) continue;
            Z = __fadd_rn(Z, s_w[j]);
            acc = __fadd_rn(acc, __fmul_rn(s_w[j], (float)D[(size_t)t * K + j]));
        }
        r = __fdiv_rn(acc, Z);                                            // Z >= 1: the cheapest candidate's weight is exp(0)
    }
    if (t < K) risk[(size_t)n * K + t] = r;
    s_risk[t] = r;
    __syncthreads();
    if (t == 0) {
        int bi = -1;
        float br = INFINITY, bc = INFINITY;
        for (int j = 0; j < K; ++j) {
            if (!s_ok[j]) continue;
            const float rj = s_risk[j], cj = s_cost[j];
            if (bi < 0 || rj < br || (rj == br && cj < bc)) { bi = j; br = rj; bc = cj; }          // (ascending j: a full tie keeps the lower index)
        }
        best[n] = bi;
        best_risk[n] = bi >= 0 ? br : INFINITY;
    }
}

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/ocr_hip.h)
// ------------------------------------------------------------------------------------------
extern "C" int ocr_edit_distance_supported(int Ka, int Kb, int N) {
    return N >= 1 && N <= 65535 && Ka >= 1 && Ka <= 65536 && Kb >= 1 && Kb <= 65536 && (long long)N * Ka * Kb <= ED_MAX_PAIRS;
}

extern "C" int ocr_edit_distance(const int* a, const int* a_len, long a_ld, long a_sn, int Ka, const int* b, const int* b_len, long b_ld, long b_sn,
                                 int Kb, int N, int ignore, int* dist, int* a_count, int* b_count, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!a || !a_len || !b || !b_len || !dist || !ocr_edit_distance_supported(Ka, Kb, N)) return OCR_ERR_INVALID;
    if (a_ld < 0 || a_sn < 0 || b_ld < 0 || b_sn < 0) return OCR_ERR_INVALID;
    if ((((uintptr_t)a | (uintptr_t)a_len | (uintptr_t)b | (uintptr_t)b_len | (uintptr_t)dist | (uintptr_t)a_count | (uintptr_t)b_count) & 3) != 0)
        return OCR_ERR_INVALID;
    const int total = N * Ka * Kb;
    const EdSet A = {a, a_len, a_ld, a_sn, Ka}, B = {b, b_len, b_ld, b_sn, Kb};
    edit_distance_kernel<<<ceil_div(total, ED_GROUP * ED_NW), ED_NT, 0, stream>>>(A, B, total, ignore, dist, a_count, b_count);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}

extern "C" int ocr_edit_stats(const int* dist, const int* ref_count, long M, long long* stats, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dist || !ref_count || !stats || M < 1 || M > ED_MAX_PAIRS) return OCR_ERR_INVALID;
    if ((((uintptr_t)dist | (uintptr_t)ref_count) & 3) != 0 || ((uintptr_t)stats & 7) != 0) return OCR_ERR_INVALID;
    edit_stats_kernel<<<1, ED_STATS_NT, 0, stream>>>(dist, ref_count, M, stats);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}

extern "C" int ocr_mbr_select(const int* dist, const float* costs, int N, int K, float* risk, int* best, float* best_risk, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dist || !costs || !risk || !best || !best_risk || N < 1 || N > 65535 || K < 1 || K > MBR_MAX_K) return OCR_ERR_INVALID;
    mbr_select_kernel<<<N, MBR_MAX_K, 0, stream>>>(dist, costs, K, risk, best, best_risk);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
