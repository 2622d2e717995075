// The k likeliest entries of every row of a cost matrix for gfx950: for costs f32 [N] rows of K entries (row stride ld >= K floats, any base
// alignment) the k smallest entries of each row under the total order (cost as a float with -0.0 == +0.0, then the lower index), ascending, with
// their indices, their own bits, their number, and optionally log_post = (-cost) - log_norm[n].  +inf entries are never returned; NaN is outside
// the contract.  This is what follows ocr_ctc_score / ocr_ctc_score_trie when the caller wants an N-best list and not the whole N x K matrix.
//
// An entry is compared as a 64-bit key: the float's bits mapped monotonically to an unsigned word (-0.0 folded onto +0.0 first, for the
// comparison only) in the high half, the index in the low half.  Keys of a row are distinct, so the k smallest are one fixed set whatever the
// order of the work; a +inf entry and an empty slot are the key of all ones, above every finite entry.  No atomics.
//
//   ctc_topk_rows_kernel   one workgroup of four waves per (segment, sample) (ocr_ctc_topk_plan cuts a row into segments so that a small N
//                          still fills the chip).  A thread loads 16 entries a round (four 16-byte loads where the base and ld allow, else four
//                          coalesced scalar rounds).  Each wave keeps its 64 smallest keys sorted, one per lane, and the k-th of them as a
//                          wave-uniform threshold: a round none of whose entries is below the threshold costs one __ballot.  Entries that pass
//                          are compacted into the wave's 64-key LDS buffer; when it would overflow it is sorted (bitonic, across lanes) and
//                          merged into the wave's best (min against the reversed list, one bitonic merge), and the threshold tightens: a
//                          descending row pays one sort per 64 entries, not one insertion per entry.  The four waves' lists are merged through
//                          LDS by wave 0.  With one segment the final outputs are written here; else the segment's k keys go to the workspace.
//   ctc_topk_merge_kernel  one workgroup per sample: the same selection over the sample's segments x k keys, then the outputs.
// Every loop bound and every branch around a cross-lane operation or a barrier is uniform: every thread reaches every barrier.  No address
// beyond costs[n * ld + K - 1] is read in any row; the selected entries' bits are read back from the row by index (signed zeros as stored).
#include "ctc_common.h"
#include <math.h>

typedef unsigned long long topk_key;
constexpr topk_key TOPK_EMPTY = ~0ull;
constexpr int TOPK_MAX_K = 1 << 20;            // entries of a row
constexpr int TOPK_MAX_SEL = 64;               // k: a wave's lanes
constexpr int TOPK_NT = 256, TOPK_NW = TOPK_NT / 64;
constexpr int TOPK_ROUND = TOPK_NT * 16;       // entries of a workgroup's round
constexpr int TOPK_ONE_WG = 2 * TOPK_ROUND;    // rows up to here are one segment whatever N
constexpr int TOPK_TARGET_WGS = 1024;          // four workgroups on each of the 256 CUs

__device__ __forceinline__ unsigned topk_hi(float v) {
    unsigned b = __float_as_uint(v);
    b = (b == 0x80000000u) ? 0u : b;                                  // -0.0 compares as +0.0
    return b ^ ((unsigned)((int)b >> 31) | 0x80000000u);              // negative: all bits flipped; else the sign bit set
}
__device__ __forceinline__ topk_key topk_make(float v, int index) {
    return v == INFINITY ? TOPK_EMPTY : ((topk_key)topk_hi(v) << 32) | (unsigned)index;
}
__device__ __forceinline__ topk_key topk_shfl(topk_key v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((topk_key)hi << 32) | lo;
}
__device__ __forceinline__ topk_key topk_shfl_xor(topk_key v, int mask) {
    const unsigned lo = __shfl_xor((unsigned)v, mask, 64), hi = __shfl_xor((unsigned)(v >> 32), mask, 64);
    return ((topk_key)hi << 32) | lo;
}
// a bitonic sequence over the wave's lanes -> ascending
__device__ __forceinline__ topk_key topk_bitonic_merge(topk_key v, int lane) {
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) {
        const topk_key o = topk_shfl_xor(v, stride);
        const bool low = (lane & stride) == 0;
        v = (low == (o < v)) ? o : v;                                 // the lower lane keeps the smaller
    }
    return v;
}
// any 64 keys -> ascending
__device__ __forceinline__ topk_key topk_sort(topk_key v, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const topk_key o = topk_shfl_xor(v, stride);
            const bool want_min = ((lane & stride) == 0) == ((lane & size) == 0);
            v = (want_min == (o < v)) ? o : v;
        }
    return v;
}
// the 64 smallest of two ascending lists, ascending
__device__ __forceinline__ topk_key topk_merge_sorted(topk_key best, topk_key other, int lane) {
    const topk_key rev = topk_shfl(other, 63 - lane);
    return topk_bitonic_merge(rev < best ? rev : best, lane);
}
// the wave's own LDS traffic: orders a lane's buffer stores before the other lanes' loads (and the loads before the next stores)
__device__ __forceinline__ void topk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A wave's selection state: best = its 64 smallest keys so far, ascending over the lanes; thr = the k-th of them; buf[0 .. count) = keys that
// passed the threshold and are not merged yet (count is wave-uniform).
struct TopkWave {
    topk_key best, thr;
    topk_key* buf;
    int count, k, lane;
    __device__ __forceinline__ void init(topk_key* buf_, int k_, int lane_) {
        best = thr = TOPK_EMPTY; buf = buf_; count = 0; k = k_; lane = lane_;
    }
    __device__ __forceinline__ void fold() {
        topk_wave_sync();
        topk_key c = lane < count ? buf[lane] : TOPK_EMPTY;
        topk_wave_sync();
        best = topk_merge_sorted(best, topk_sort(c, lane), lane);
        thr = topk_shfl(best, k - 1);
        count = 0;
    }
    // called by the whole wave, a key per lane (TOPK_EMPTY: nothing to offer)
    __device__ __forceinline__ void offer(topk_key key) {
        bool pass = key < thr;
        unsigned long long bal = __ballot(pass);
        if (!bal) return;
        if (count + __popcll(bal) > 64) {
            fold();
            pass = key < thr;
            bal = __ballot(pass);
        }
        if (pass) buf[count + __popcll(bal & ((1ull << lane) - 1))] = key;
        count += __popcll(bal);
    }
};

// The workgroup's result from its waves' states: every wave folds its buffer, wave 0 merges the four lists -> the workgroup's 64 smallest keys,
// ascending, in wave 0's lanes (other waves: their own list).  s_keys = TOPK_NW * 64 keys, the waves' buffers included.  Two barriers.
__device__ __forceinline__ topk_key topk_block_merge(TopkWave& w, topk_key* s_keys, int wave) {
    w.fold();
    __syncthreads();                                      // (the buffers are dead: s_keys is reused for the lists)
    s_keys[wave * 64 + w.lane] = w.best;
    __syncthreads();
    topk_key best = w.best;
    if (wave == 0) {
#pragma unroll
        for (int o = 1; o < TOPK_NW; ++o) {
            const topk_key rev = s_keys[o * 64 + 63 - w.lane];
            best = topk_bitonic_merge(rev < best ? rev : best, w.lane);
        }
    }
    return best;
}

// the outputs of sample n from the sorted keys in one wave's lanes
__device__ __forceinline__ void topk_write(topk_key key, const float* __restrict__ row, const float* __restrict__ log_norm, int n, int k, int lane,
                                           int* __restrict__ index, float* __restrict__ cost, float* __restrict__ log_post, int* __restrict__ count) {
    const bool hit = lane < k && key != TOPK_EMPTY;
    const unsigned long long bal = __ballot(hit);
    if (lane < k) {
        const int i = hit ? (int)(unsigned)key : -1;
        const float c = hit ? row[i] : INFINITY;          // the entry's own bits
        const size_t o = (size_t)n * k + lane;
        index[o] = i;
        cost[o] = c;
        if (log_post) log_post[o] = hit ? __fsub_rn(-c, log_norm[n]) : NEG_INF;
    }
    if (lane == 0) count[n] = __popcll(bal);
}

// VEC: the base is 16-byte aligned and ld % 4 == 0, so every row is; segment starts are multiples of TOPK_ROUND
template <bool VEC>
__global__ __launch_bounds__(TOPK_NT) void ctc_topk_rows_kernel(const float* __restrict__ costs, long ld, int K, int k, int segments, int segment_len,
                                                                const float* __restrict__ log_norm, int* __restrict__ index, float* __restrict__ cost,
                                                                float* __restrict__ log_post, int* __restrict__ count, topk_key* __restrict__ partial) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x, n = blockIdx.y;
    const float* row = costs + (size_t)n * ld;
    const int start = seg * segment_len, end = min(K, start + segment_len);
    __shared__ topk_key s_keys[TOPK_NW * 64];
    TopkWave w;
    w.init(s_keys + wave * 64, k, lane);

    for (int off = start; off < end; off += TOPK_ROUND) {          // (uniform: a thread past the end offers +inf)
        float v[16];
        int at[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if constexpr (VEC) {
                const int i0 = off + u * (TOPK_NT * 4) + tid * 4;
                f32x4 x = {INFINITY, INFINITY, INFINITY, INFINITY};
                if (i0 + 4 <= end) x = *(const f32x4*)(row + i0);
                else {
                    if (i0 < end) x.x = row[i0];
                    if (i0 + 1 < end) x.y = row[i0 + 1];
                    if (i0 + 2 < end) x.z = row[i0 + 2];
                }
                v[4 * u] = x.x; v[4 * u + 1] = x.y; v[4 * u + 2] = x.z; v[4 * u + 3] = x.w;
#pragma unroll
                for (int q = 0; q < 4; ++q) at[4 * u + q] = i0 + q;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = off + (4 * u + q) * TOPK_NT + tid;
                    v[4 * u + q] = i < end ? row[i] : INFINITY;
                    at[4 * u + q] = i;
                }
            }
        }
        // the round's filter: on ordinary data no entry is at or below the threshold's cost
        unsigned least = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < 16; ++j) least = min(least, v[j] == INFINITY ? 0xffffffffu : topk_hi(v[j]));
        if (!__ballot(least <= (unsigned)(w.thr >> 32) && least != 0xffffffffu)) continue;
#pragma unroll
        for (int j = 0; j < 16; ++j) w.offer(topk_make(v[j], at[j]));
    }
    const topk_key best = topk_block_merge(w, s_keys, wave);
    if (wave != 0) return;                                // (after the last barrier)
    if (segments == 1) topk_write(best, row, log_norm, n, k, lane, index, cost, log_post, count);
    else if (lane < k) partial[((size_t)n * segments + seg) * k + lane] = best;
}

__global__ __launch_bounds__(TOPK_NT) void ctc_topk_merge_kernel(const float* __restrict__ costs, long ld, int k, int segments,
                                                                 const float* __restrict__ log_norm, int* __restrict__ index, float* __restrict__ cost,
                                                                 float* __restrict__ log_post, int* __restrict__ count, const topk_key* __restrict__ partial) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x, M = segments * k;
    const topk_key* keys = partial + (size_t)n * M;
    __shared__ topk_key s_keys[TOPK_NW * 64];
    TopkWave w;
    w.init(s_keys + wave * 64, k, lane);
    for (int off = 0; off < M; off += TOPK_NT) {
        const int i = off + tid;
        w.offer(i < M ? keys[i] : TOPK_EMPTY);
    }
    const topk_key best = topk_block_merge(w, s_keys, wave);
    if (wave == 0) topk_write(best, costs + (size_t)n * ld, log_norm, n, k, lane, index, cost, log_post, count);
}

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/ocr_hip.h)
// ------------------------------------------------------------------------------------------
extern "C" int ocr_ctc_topk_supported(int K, int k) { return K >= 1 && K <= TOPK_MAX_K && k >= 1 && k <= TOPK_MAX_SEL; }

// How the launch cuts a row: one segment where a workgroup's two rounds hold it or the samples alone make TOPK_TARGET_WGS workgroups; else as
// many segments as that target asks for, none shorter than a round, each a whole number of rounds.
extern "C" int ocr_ctc_topk_plan(int N, int K, int k, int* segments, int* segment_len) {
    if (!segments || !segment_len || N < 1 || N > 65535 || !ocr_ctc_topk_supported(K, k)) return OCR_ERR_INVALID;
    int want = 1;
    if (K > TOPK_ONE_WG) want = min(ceil_div(K, TOPK_ROUND), ceil_div(TOPK_TARGET_WGS, N));
    const int len = ceil_div(ceil_div(K, want), TOPK_ROUND) * TOPK_ROUND;
    *segments = ceil_div(K, len);
    *segment_len = len;
    return OCR_OK;
}
// the segments' keys: 0 bytes for a one-segment plan
extern "C" int ocr_ctc_topk_workspace_size(int N, int K, int k, size_t* bytes) {
    int segments = 0, len = 0;
    if (!bytes || ocr_ctc_topk_plan(N, K, k, &segments, &len) != OCR_OK) return OCR_ERR_INVALID;
    *bytes = segments > 1 ? ctc_align256((size_t)N * segments * k * sizeof(topk_key)) : 0;
    return OCR_OK;
}
extern "C" int ocr_ctc_topk(const float* costs, long ld, int N, int K, int k, const float* log_norm, int* index, float* cost, float* log_post,
                            int* count, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!costs || !index || !cost || !count || (log_post && !log_norm)) return OCR_ERR_INVALID;
    int segments = 0, len = 0;
    size_t need = 0;
    if (ocr_ctc_topk_plan(N, K, k, &segments, &len) != OCR_OK || ocr_ctc_topk_workspace_size(N, K, k, &need) != OCR_OK) return OCR_ERR_INVALID;
    if (ld < K || ((uintptr_t)costs & 3) != 0) return OCR_ERR_INVALID;
    if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7) != 0)) return OCR_ERR_INVALID;
    topk_key* partial = (topk_key*)workspace;

    const dim3 grid(segments, N);
    if (((uintptr_t)costs & 15) == 0 && ld % 4 == 0)
        ctc_topk_rows_kernel<true><<<grid, TOPK_NT, 0, stream>>>(costs, ld, K, k, segments, len, log_norm, index, cost, log_post, count, partial);
    else
        ctc_topk_rows_kernel<false><<<grid, TOPK_NT, 0, stream>>>(costs, ld, K, k, segments, len, log_norm, index, cost, log_post, count, partial);
    OCR_CHECK_LAUNCH();
    if (segments > 1) {
        ctc_topk_merge_kernel<<<N, TOPK_NT, 0, stream>>>(costs, ld, k, segments, log_norm, index, cost, log_post, count, partial);
        OCR_CHECK_LAUNCH();
    }
    return OCR_OK;
}
