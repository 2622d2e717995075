// Lexicon scoring under CTC on a prefix tree, for gfx950: the costs ocr_ctc_score (ctc_score.hip) gives, for dictionaries of up to 2^20 words.
// ctc_score.hip runs the 2L + 1 slots of every word for every frame, one wave per (sample, word); words of a dictionary share prefixes, and the
// alpha recursion of a prefix does not depend on what follows it, so here every NODE of the lexicon's prefix tree runs it once:
//     pnb_t(v) = y_t[c_v]   + lse(pnb_{t-1}(v), pb_{t-1}(p_v), [c_v != c_{p_v}] pnb_{t-1}(p_v))        alpha at the node's label slot
//     pb_t(v)  = y_t[blank] + lse(pb_{t-1}(v), pnb_{t-1}(v))                                           alpha at the blank slot behind it
// with pb_0(root) = y_0[blank], pnb_0(v) = y_0[c_v] for the root's children and -inf elsewhere; a word that ends in v costs
// -lse(pb_{Tn-1}(v), pnb_{Tn-1}(v)).  These are ctc_score_cands_kernel's updates slot for slot, with lse3_flat and its argument order, so a
// finite cost can equal ocr_ctc_score's bit for bit.  A word with L + repeats > Tn comes out -inf by itself: cost +inf.
//
// Host side (no GPU): ocr_ctc_trie_build sorts the words and cuts the sorted order into contiguous ranges ("chunks") whose own tries have at
// most chunk_nodes nodes, the root and the ancestors a range shares with its neighbours included: a shared prefix chain is built again in
// every chunk that needs it, which is the price of workgroups that never communicate.
//
// Three launches, ordered by the stream: ctc_common.h's rows launch (lse[t][n], as ocr_ctc_score), ctc_trie_kernel with one workgroup per
// (chunk, sample), and ctc_common.h's arg-min / log-normaliser launch.
#include "ctc_common.h"
#include <math.h>

#include <algorithm>
#include <vector>

constexpr int TRIE_MAX_K = 1 << 20;
constexpr int TRIE_MAX_LABEL = 255;
constexpr int TRIE_CAP = 8192;           // nodes of a chunk: 1024 threads x 8 nodes; two LDS buffers of (pb, pnb) = 16 bytes a node, 128 KiB
// a node record: label in bits 0..13 (C <= 16384), the parent's local index in bits 14..26 (< TRIE_CAP), bit 27 = the node may take its
// parent's non-blank mass (its label differs from the parent's; never set for the root's children)
constexpr int TRIE_LABEL_BITS = 14, TRIE_PARENT_BITS = 13;
static_assert(SCORE_MAX_C <= (1 << TRIE_LABEL_BITS) && TRIE_CAP <= (1 << TRIE_PARENT_BITS), "node record fields");

// One workgroup per (chunk, sample).  Thread tid owns the nodes tid, tid + NT, ... (VT of them): record, pb and pnb in registers; before every
// frame the values of the frame before are published in one of two LDS buffers (one barrier a frame: the buffer written for frame t + 1 was last
// read for frame t - 1, behind the barrier of frame t) and a node reads its parent's pair from there.  Per frame a thread gathers
// act[t][n][label] for its nodes; the blank's logit and lse[t][n] are one address each; the loads of frame t + 1 are issued before the
// log-add-exp of frame t.  cap = nodes a buffer holds (the lexicon's largest chunk, <= NT * VT).  Every thread reaches every barrier: the only
// return before the end is taken by the whole workgroup (Tn <= 0) ahead of the first one.
template <int NT, int VT>
__global__ __launch_bounds__(NT) void ctc_trie_kernel(const float* __restrict__ act, const float* __restrict__ lse, const int* __restrict__ input_len,
                                                      const int* __restrict__ nodes, const int* __restrict__ chunk_node_start,
                                                      const int* __restrict__ chunk_word_start, const int* __restrict__ word_node,
                                                      const int* __restrict__ word_index, int T, int N, int C, int K, int blank, int cap,
                                                      float* __restrict__ costs) {
    extern __shared__ __attribute__((aligned(16))) float2 trie_buf[];          // [2][cap] (pb, pnb)
    const int tid = threadIdx.x, ch = blockIdx.x, n = blockIdx.y;
    const int n0 = chunk_node_start[ch], w0 = chunk_word_start[ch], w1 = chunk_word_start[ch + 1];
    const int nn = max(min(chunk_node_start[ch + 1] - n0, cap), 0);           // (a chunk never exceeds cap: the host refuses such a lexicon)
    const int Tn = min(input_len[n], T);
    float* out = costs + (size_t)n * K;
    if (Tn <= 0) {                                        // (the whole workgroup: n is the workgroup's)
        for (int w = w0 + tid; w < w1; w += NT) {
            const int idx = word_index[w];
            if ((unsigned)idx < (unsigned)K) out[idx] = INFINITY;
        }
        return;
    }

    // this thread's nodes.  A slot past the chunk, and the root's label slot, stay -inf; their gathers read the blank's logit (one address).
    int lab[VT], par[VT];
    bool has[VT], lbl[VT], skip[VT];
#pragma unroll
    for (int j = 0; j < VT; ++j) {
        const int v = j * NT + tid;
        has[j] = v < nn;
        const int rec = has[j] ? nodes[n0 + v] : 0;
        const int c = rec & ((1 << TRIE_LABEL_BITS) - 1), p = (rec >> TRIE_LABEL_BITS) & ((1 << TRIE_PARENT_BITS) - 1);
        lbl[j] = has[j] && v > 0 && c < C && p < v;       // (what the builder writes always passes; nothing else is used as an index)
        lab[j] = lbl[j] ? c : blank;
        par[j] = lbl[j] ? p : 0;
        skip[j] = lbl[j] && ((rec >> (TRIE_LABEL_BITS + TRIE_PARENT_BITS)) & 1);
    }

    const size_t tstride = (size_t)N * C;
    const float* a_n = act + (size_t)n * C;
    const float* lse_n = lse + n;
    float g[VT], gb, gl;
#define TRIE_LOAD(t_)                                                                                          \
    do {                                                                                                       \
        const float* row_ = a_n + (size_t)(t_) * tstride;                                                      \
        gb = row_[blank]; gl = lse_n[(size_t)(t_) * N];                                                        \
        _Pragma("unroll") for (int j = 0; j < VT; ++j) g[j] = row_[lab[j]];                                    \
    } while (0)
#define TRIE_LOGY()                                                                                            \
    _Pragma("unroll") for (int j = 0; j < VT; ++j) {                                                           \
        lyl[j] = lbl[j] ? g[j] - gl : NEG_INF;                                                                 \
        lyb[j] = has[j] ? gb - gl : NEG_INF;                                                                   \
    }
    float pb[VT], pnb[VT], lyl[VT], lyb[VT];
    TRIE_LOAD(0);
    TRIE_LOGY();
#pragma unroll
    for (int j = 0; j < VT; ++j) {
        pb[j] = (j == 0 && tid == 0) ? lyb[j] : NEG_INF;            // the root's blank slot (slot 0 of every word)
        pnb[j] = (lbl[j] && par[j] == 0) ? lyl[j] : NEG_INF;        // slot 1 of the words that begin with this label
    }
    if (Tn > 1) { TRIE_LOAD(1); TRIE_LOGY(); }
    int cur = 0;
    for (int t = 1; t < Tn; ++t) {
        float2* sb = trie_buf + (size_t)cur * cap;
#pragma unroll
        for (int j = 0; j < VT; ++j)
            if (has[j]) sb[j * NT + tid] = make_float2(pb[j], pnb[j]);
        __syncthreads();
        TRIE_LOAD(min(t + 1, Tn - 1));                    // frame t + 1, in flight during the step below
        float npb[VT], npnb[VT];
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const float2 p = sb[par[j]];
            npnb[j] = lse3_flat(pnb[j], p.x, skip[j] ? p.y : NEG_INF) + lyl[j];
            npb[j] = lse3_flat(pb[j], pnb[j], NEG_INF) + lyb[j];
        }
#pragma unroll
        for (int j = 0; j < VT; ++j) { pb[j] = npb[j]; pnb[j] = npnb[j]; }
        TRIE_LOGY();
        cur ^= 1;
    }
#undef TRIE_LOAD
#undef TRIE_LOGY
    float2* sb = trie_buf + (size_t)cur * cap;
#pragma unroll
    for (int j = 0; j < VT; ++j)
        if (has[j]) sb[j * NT + tid] = make_float2(pb[j], pnb[j]);
    __syncthreads();
    // this chunk's words: the cost of the terminal node into the caller's column; +inf for an invalid word (node -1) and an infeasible one
    for (int w = w0 + tid; w < w1; w += NT) {
        const int v = word_node[w], idx = word_index[w];
        float c = INFINITY;
        if ((unsigned)v < (unsigned)nn) {
            const float e1 = sb[v].x, e2 = sb[v].y, m = fmaxf(e1, e2);
            if (m != NEG_INF) c = -(m + logf(expf(e1 - m) + expf(e2 - m)));
        }
        if ((unsigned)idx < (unsigned)K) out[idx] = c;
    }
}

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/ocr_hip.h)
// ------------------------------------------------------------------------------------------
extern "C" int ocr_ctc_trie_chunk_capacity(void) { return TRIE_CAP; }
extern "C" int ocr_ctc_trie_supported(int alphabet_size, int max_time, int num_words) {
    return alphabet_size >= 1 && alphabet_size <= SCORE_MAX_C && max_time >= 1 && num_words >= 1 && num_words <= TRIE_MAX_K;
}
// the lse[T][N] table, as ocr_ctc_score_workspace_size
extern "C" int ocr_ctc_trie_workspace_size(int alphabet_size, int max_time, int minibatch, size_t* bytes) {
    if (!bytes || minibatch <= 0 || !ocr_ctc_trie_supported(alphabet_size, max_time, 1) || (long)minibatch * max_time > 0x7fffffffL)
        return OCR_ERR_INVALID;
    *bytes = ctc_align256((size_t)minibatch * max_time * sizeof(float));
    return OCR_OK;
}

// Host code.  Valid words in lexicographic order (a prefix before its extensions, equal words by index); the invalid ones ahead of them, in
// chunk 0, with node -1.  A chunk is closed when the next word's new nodes would not fit; its successor starts again from the root.
extern "C" int ocr_ctc_trie_build(const int* words, const int* lengths, int num_words, int max_label_len, int alphabet_size, int blank_label,
                                  int chunk_nodes, int* num_chunks, int* num_nodes, int* nodes, int* chunk_node_start, int* chunk_word_start,
                                  int* word_node, int* word_index) {
    const int K = num_words, Lmax = max_label_len, C = alphabet_size;
    if (!lengths || !num_chunks || !num_nodes || K < 1 || K > TRIE_MAX_K || Lmax < 0 || (!words && Lmax > 0)) return OCR_ERR_INVALID;
    if (C < 1 || C > SCORE_MAX_C || blank_label < 0 || blank_label >= C || chunk_nodes < 1 || chunk_nodes > TRIE_CAP) return OCR_ERR_INVALID;
    const bool fill = nodes != nullptr;
    if (fill && (!chunk_node_start || !chunk_word_start || !word_node || !word_index)) return OCR_ERR_INVALID;
    const int cap_chunks = *num_chunks, cap_nodes = *num_nodes;          // (read by the fill pass only: what the size query returned)

    std::vector<int> order, bad;
    order.reserve(K);
    int deepest = 0;
    for (int k = 0; k < K; ++k) {
        const int L = lengths[k];
        bool ok = L >= 0 && L <= Lmax && L <= TRIE_MAX_LABEL;
        const int* w = words + (size_t)k * Lmax;
        for (int i = 0; ok && i < L; ++i) ok = (unsigned)w[i] < (unsigned)C && w[i] != blank_label;
        if (ok) { order.push_back(k); deepest = std::max(deepest, L); }
        else bad.push_back(k);
    }
    if (chunk_nodes < deepest + 1) return OCR_ERR_INVALID;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        const int* wa = words + (size_t)a * Lmax;
        const int* wb = words + (size_t)b * Lmax;
        const int la = lengths[a], lb = lengths[b], l = std::min(la, lb);
        for (int i = 0; i < l; ++i)
            if (wa[i] != wb[i]) return wa[i] < wb[i];
        return la != lb ? la < lb : a < b;
    });

    long total = 0;                      // nodes of the closed chunks
    int chunks = 0, cn = 1, pos = 0;     // the open chunk: its index, its nodes so far (the root), the next position of the sorted order
    auto open_chunk = [&]() -> bool {
        if (fill) {
            if (chunks >= cap_chunks || total + 1 > cap_nodes) return false;
            chunk_node_start[chunks] = (int)total;
            chunk_word_start[chunks] = pos;
            nodes[total] = blank_label;                  // the root: no label of its own, its own parent
        }
        cn = 1;
        return true;
    };
    if (!open_chunk()) return OCR_ERR_INVALID;
    for (int k : bad) {
        if (fill) { word_node[pos] = -1; word_index[pos] = k; }
        ++pos;
    }
    int path[TRIE_MAX_LABEL + 1];        // path[d] = the open chunk's node of the previous word's prefix of d + 1 labels
    const int* prev = nullptr;
    int prev_len = 0;
    for (int k : order) {
        const int* w = words + (size_t)k * Lmax;
        const int L = lengths[k];
        int l = 0;
        if (prev) while (l < L && l < prev_len && w[l] == prev[l]) ++l;
        if (cn + (L - l) > chunk_nodes) {                // (never the first word of a chunk: deepest + 1 <= chunk_nodes)
            total += cn;
            ++chunks;
            if (!open_chunk()) return OCR_ERR_INVALID;
            l = 0;
        }
        for (int d = l; d < L; ++d) {
            if (fill) {
                if (total + cn + 1 > cap_nodes) return OCR_ERR_INVALID;
                const int parent = d ? path[d - 1] : 0;
                nodes[total + cn] = w[d] | (parent << TRIE_LABEL_BITS) | ((d && w[d] != w[d - 1]) ? 1 << (TRIE_LABEL_BITS + TRIE_PARENT_BITS) : 0);
            }
            path[d] = cn++;
        }
        if (fill) { word_node[pos] = L ? path[L - 1] : 0; word_index[pos] = k; }
        ++pos;
        prev = w;
        prev_len = L;
    }
    total += cn;
    ++chunks;
    if (total > 0x7fffffffL) return OCR_ERR_INVALID;
    if (fill) { chunk_node_start[chunks] = (int)total; chunk_word_start[chunks] = pos; }
    *num_chunks = chunks;
    *num_nodes = (int)total;
    return OCR_OK;
}

template <int NT, int VT>
static void ctc_trie_launch(const float* act, const float* lse, const int* il, const int* nodes, const int* cns, const int* cws, const int* wn,
                            const int* wi, int chunks, int T, int N, int C, int K, int blank, int cap, float* costs, hipStream_t stream) {
    ctc_trie_kernel<NT, VT><<<dim3(chunks, N), NT, (size_t)2 * cap * sizeof(float2), stream>>>(act, lse, il, nodes, cns, cws, wn, wi, T, N, C, K, blank,
                                                                                              cap, costs);
}

extern "C" int ocr_ctc_score_trie(const float* activations, const int* input_lengths, const int* nodes, const int* chunk_node_start,
                                  const int* chunk_word_start, const int* word_node, const int* word_index, int num_chunks, int chunk_nodes,
                                  int alphabet_size, int minibatch, int max_time, int num_words, int blank_label, float* costs, int* best,
                                  float* best_cost, float* log_norm, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!activations || !input_lengths || !nodes || !chunk_node_start || !chunk_word_start || !word_node || !word_index || !costs || !workspace)
        return OCR_ERR_INVALID;
    const int outs = (best != nullptr) + (best_cost != nullptr) + (log_norm != nullptr);
    if (outs != 0 && outs != 3) return OCR_ERR_INVALID;
    if (!ocr_ctc_trie_supported(alphabet_size, max_time, num_words)) return OCR_ERR_INVALID;
    if (blank_label < 0 || blank_label >= alphabet_size || chunk_nodes < 1 || chunk_nodes > TRIE_CAP) return OCR_ERR_INVALID;
    if (num_chunks < 1 || num_chunks > num_words + 1) return OCR_ERR_INVALID;          // (every chunk but the first holds a word)
    if (minibatch > 65535) return OCR_ERR_INVALID;        // the trie launch has the sample in grid.y
    size_t need = 0;
    if (ocr_ctc_trie_workspace_size(alphabet_size, max_time, minibatch, &need) != OCR_OK || workspace_bytes < need) return OCR_ERR_INVALID;
    const int C = alphabet_size, N = minibatch, T = max_time, K = num_words;
    float* lse = (float*)workspace;

    ctc_score_rows(activations, input_lengths, T, N, C, lse, stream);
    OCR_CHECK_LAUNCH();

    // the smallest form whose registers hold the largest chunk, so that no register slot idles in a full chunk: 256 threads x 1 / 2 / 4 nodes,
    // 512 x 8, 1024 x 8.  The LDS buffers are sized by chunk_nodes itself (16 bytes a node).  Measured at N = 64, T = 63: chunks of
    // 512 and 1024 nodes are the fastest, 4096 costs 4 .. 15 % and 8192 20 .. 40 % more (one 1024-thread workgroup a CU); lexicon.py's
    // default is 1024, which is the best size where the gathers miss (6625 classes, sparse words)
#define TRIE_RUN(NT, VT)                                                                                                                   \
    ctc_trie_launch<NT, VT>(activations, lse, input_lengths, nodes, chunk_node_start, chunk_word_start, word_node, word_index, num_chunks, T, N, C, K, \
                            blank_label, chunk_nodes, costs, stream)
    if (chunk_nodes <= 256) TRIE_RUN(256, 1);
    else if (chunk_nodes <= 256 * 2) TRIE_RUN(256, 2);
    else if (chunk_nodes <= 256 * 4) TRIE_RUN(256, 4);
    else if (chunk_nodes <= 512 * 8) TRIE_RUN(512, 8);
    else TRIE_RUN(1024, 8);
#undef TRIE_RUN
    OCR_CHECK_LAUNCH();

    if (outs == 3) {
        ctc_score_best(costs, N, K, best, best_cost, log_norm, stream);
        OCR_CHECK_LAUNCH();
    }
    return OCR_OK;
}
