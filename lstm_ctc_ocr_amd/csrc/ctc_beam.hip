// CTC prefix beam search on the device — the decoder the reference actually runs:
//   tf.nn.ctc_beam_search_decoder(logits, seq_len, merge_repeated=True)   (lib/networks/network.py:656, lib/lstm/test.py:30)
// with TF's defaults beam_width = 100, top_paths = 1 and TF's conventions: BLANK = num_classes - 1, per-beam
// (p_blank, p_label) in log space, a child that is already in the beam receives its parent's mass through the
// "parent active" update, children that are not in the beam compete with the current leaves, the `beam_width` best
// totals survive each frame, and merge_repeated collapses adjacent equal labels of the emitted sequence.
// (TF's CPU op streams candidates through a bounded heap; on per-frame log-softmax scores that is exactly "top
// beam_width of {updated leaves} U {new children}", which is what is computed here — ties aside.)
//
// One workgroup (256 threads) per sample; per frame: log-softmax row -> leaf update -> child scores in LDS ->
// exact K-th-largest threshold by 32-step bisection on the order-preserving integer image of the floats -> ordered
// compaction into the next beam -> trie bookkeeping (node pool in a caller-owned workspace).  This path runs at
// validation / test time only; it is latency-, not throughput-critical.
//
// Node identity is per PREFIX, for the whole decode: a beam entry finds its parent's slot through nslot[npar[node]], and that is the
// only thing that tells step (b) which entry feeds it and step (c) which children need no candidate.  A prefix P can drop out of the
// beam while its extension Q = P + c stays, and come back frames later as a child of its own parent (flat logits do this all the time,
// peaky ones hardly ever).  If P then got a fresh node, Q would still hang off the old one: it would never receive P's mass again and
// (P, c) would be scored as a new candidate - a second copy of Q with part of the mass - where TF keeps a child in its parent's
// `children` map for good and restarts the same object from zero.  So step (f) looks every admitted child (parent node, label) up among
// the existing nodes (one pass over the pool per frame) and puts it back on its node with (p_blank, p_label) = (0, candidate score); only
// a prefix never seen before takes a new node.  The pool bound T*K + 2 holds all the more.
//
// Two kernels share that body.  The TABLE kernel (WIDE = false) scores every (beam entry, class) pair and answers "is child (b, c)
// already in the beam" from a 16-bit [K][C] table: about 6*K*C bytes of LDS, which at K = 100 ends at 259 classes.  The WIDE kernel
// (WIDE = true) has no K*C term.  Per frame it first selects S, the M = min(K + 1, C - 1) non-blank classes with the largest lp (ties
// at the boundary to the lowest class index), and scores only the pairs (b, S[j]).  That loses nothing: a new child b + c scores
// lp[c] + tot[b] (or lp[c] + pb[b] <= that when c == last[b]); for c outside S at least K of the entries b + c', c' in S, c' != last[b],
// score at least as much whether they are new or already in the beam, so b + c is not among the K best (ties aside, as above).  A child
// that IS in the beam needs no candidate whatever its class: it gets its parent's mass in the leaf update (b).  S is kept in ascending
// class order, so candidates keep the relative order of b*C + c and the tie rule of step (e) is the table kernel's.  The in-beam
// question is answered without a table: each beam entry whose parent is in the beam looks its own label up in S (binary search) and
// cancels that one candidate.  LDS: 4*C + 4*(K + K*M) + 4*M bytes plus the beam arrays, 136 KB at C = 16384, K = 128.
//
// LM = true (table kernel only) is ocr_ctc_beam_decode_lm: the search is steered by a deterministic weighted automaton over the labels
// (next[state][class], weight[state][class], final[state]; -inf = forbidden).  Every alignment that collapses to a prefix P holds the same
// characters, so the fused score factorises exactly: total(P) = log p_beam(P) + W(P), W(P) the sum of the weights along P's state sequence.
// The state is a function of the prefix, so it lives on the prefix's node: node_state / node_w (the weight the last character paid) are
// written once where step (f) allocates the node, and a prefix that re-enters the beam on its old node finds them there.  New children pay
// their weight in step (c), the mass an in-beam child takes from its in-beam parent pays the child's node_w in step (b), the repeat term
// pnb[s] and the blank term pay nothing.  Pruning ranks by total; the final ranking adds final[state].  A transition is forbidden when its
// weight is not finite or its next state lies outside [0, num_states): every state the kernel holds is in range, so no table content
// makes it read outside the tables.
//
// LM = true with WIDE = true is ocr_ctc_beam_decode_lm_sparse: the same terms on the wide kernel, the automaton in the sparse form with failure
// (back-off) arcs of automaton.SparseLabelAutomaton.  Its size follows the arcs that exist, so a bigram or a lexicon trie over thousands of
// classes fits.  sparse_step walks at most SPARSE_MAX_HOPS back-off hops, each a binary search among the state's arcs; every arc range is
// clamped to [0, num_arcs], every arc_next and backoff is bounds-checked and the hop count is capped, so no array content makes the kernel
// read outside the arrays or loop.  With weights in the search the wide kernel's "the K + 1 likeliest classes lose nothing" no longer
// holds (a class outside S may carry a large weight), so here the selection is part of the specification: new children are restricted to
// the M = min(cutoff, C - 1) likeliest non-blank classes of the frame, the acoustic pruning of every practical decoder.  A child that is
// in the beam still takes its parent's mass in step (b) whatever its class.
#include "common.h"
#include <float.h>
#include <math.h>
#include <type_traits>

#define BEAM_MAX 128
#define BEAM_WIDE_MAX_C 16384        // the wide kernel's promise: 2 <= C <= 16384 for every K <= BEAM_MAX (node_label is a short)
#define BEAM_LDS_LIMIT (160 * 1024)
#define NEGINF (-INFINITY)

__device__ __forceinline__ float blse(float a, float b) {
    float m = fmaxf(a, b);
    if (m == NEGINF) return NEGINF;
    return m + logf(expf(a - m) + expf(b - m));
}
// order-preserving float -> uint key (larger float <=> larger key; -inf is the smallest finite-ordered key)
__device__ __forceinline__ unsigned fkey(float f) {
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct BeamArgs {
    const float* act; const int* input_len; int T, N, C, K, merge_repeated, pad_value;
    int* out; int* out_len; float* neg_log_prob;
    int* node_parent; short* node_label; int* node_slot;     // per sample: T*K + 2 entries
    int blank, top_paths; int* count;                        // n-best entry only (NBEST = true)
};
// the fused entry's operands ride behind the others, so the instances without LM keep their kernel arguments
struct BeamLmArgs : BeamArgs {
    const int* lm_next; const float* lm_weight; const float* lm_final; int num_states;      // [H][C], [H][C], [H]: the caller's class ids
    int* node_state; float* node_w;                          // per sample: T*K + 2 entries, beside node_parent / node_label / node_slot
    float* lm_score;
};
__device__ __forceinline__ bool lm_finite(float w) { return fabsf(w) <= FLT_MAX; }       // false for -inf, +inf and NaN
// the sparse fused entry's operands: an argument struct of its own, so every other instance keeps its kernel arguments
struct BeamSparseArgs : BeamArgs {
    const int* arc_begin; const int* arc_label; const int* arc_next; const float* arc_weight;      // [H + 1], [A], [A], [A]: the caller's class ids
    const int* backoff; const float* backoff_weight; const float* lm_final;                        // [H], [H], [H]
    int num_states, num_arcs, cutoff;
    int* node_state; float* node_w;
    float* lm_score;
};
#define SPARSE_MAX_HOPS 8
// Reading the caller's class c in state s (0 <= s < num_states): true and (w, next) when the transition exists.  The arcs of s are searched
// for c (lower bound by bisection; labels that are not ascending only make the search miss); a miss retries in backoff[s] after paying
// backoff_weight[s], at most SPARSE_MAX_HOPS times.  w = ((bw_1 + bw_2) + ..) + arc_weight in float32, which the host reproduces to the bit.
__device__ __forceinline__ bool sparse_step(const BeamSparseArgs& a, int s, int c, float& w, int& next) {
    float acc = 0.f;
    for (int hops = 0;; ++hops) {
        int lo = min(max(a.arc_begin[s], 0), a.num_arcs);
        const int end = min(max(a.arc_begin[s + 1], 0), a.num_arcs);
        int hi = max(end, lo);                               // an inverted range is empty
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.arc_label[mid] < c) lo = mid + 1; else hi = mid; }
        if (lo < end && a.arc_label[lo] == c) {
            const float aw = a.arc_weight[lo];
            const unsigned nx = (unsigned)a.arc_next[lo];
            w = acc + aw; next = (int)nx;
            return lm_finite(aw) && lm_finite(w) && nx < (unsigned)a.num_states;
        }
        const unsigned bo = (unsigned)a.backoff[s];
        const float bw = a.backoff_weight[s];
        if (hops == SPARSE_MAX_HOPS || bo >= (unsigned)a.num_states || !lm_finite(bw)) return false;
        acc += bw; s = (int)bo;
    }
}

// NBEST = true is ocr_ctc_beam_decode_nbest: the caller's blank is any class and the `top_paths` best leaves are emitted.  Inside the
// kernel the blank stays the LAST class: the log-softmax row is stored through the monotone re-indexing  k -> k (k < blank),
// C - 1 (k == blank), k - 1 (k > blank), and a label is translated back where a path is emitted.  The re-indexing keeps the order of the
// non-blank classes, so every "lowest class index" / "lowest candidate index" tie rule picks the class it would pick in the caller's
// numbering, and for blank == C - 1 it is the identity.  NBEST = false is ocr_ctc_beam_decode as it always was (no re-indexing in its
// instances, thread 0 emits the best leaf).
// LM = true is ocr_ctc_beam_decode_lm (see the header): NBEST's re-indexing and emission, the automaton's terms in steps (b), (c), (f) and in
// the final ranking.  Its tables are indexed by the caller's class ids: internal class c is the caller's  c < blank ? c : c + 1.
template <bool WIDE, bool NBEST, bool LM = false>
__global__ __launch_bounds__(256) void ctc_beam_kernel(std::conditional_t<LM, std::conditional_t<WIDE, BeamSparseArgs, BeamLmArgs>, BeamArgs> a) {
    static_assert(!LM || NBEST, "the fused search emits through the n-best path");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, K = a.K, blank = C - 1;
    const int Tn = min(a.input_len[n], a.T);
    const int pool = a.T * K + 2;
    int Msel = WIDE ? min(K + 1, C - 1) : C;              // candidate classes per beam entry (the table kernel scores all C)
    if constexpr (WIDE && LM) Msel = min(a.cutoff, C - 1);   // the sparse fused entry: the caller's acoustic cutoff, 1 <= cutoff <= K + 1
    const int M = Msel;
    int* npar = a.node_parent + (size_t)n * pool;
    short* nlab = a.node_label + (size_t)n * pool;
    int* nslot = a.node_slot + (size_t)n * pool;

    // ---- LDS carve-up
    float* lp = (float*)smem_raw;                         // [C]
    float* cand = lp + ((C + 3) & ~3);                    // [K + K*M]
    short* table = (short*)(cand + K + K * M);            // table kernel: [K][C] child slot of (parent slot, label) or -1
    int* sel_cls = (int*)(cand + K + K * M);              // wide kernel: S[M], the frame's candidate classes in ascending order
    int* b_node = WIDE ? sel_cls + M : (int*)(table + ((K * C + 1) & ~1));     // beam arrays, two generations
    int* b_last = b_node + 2 * BEAM_MAX;
    int* b_ps = b_last + 2 * BEAM_MAX;                    // slot of the parent entry if it is in the beam, else -1
    float* b_pb = (float*)(b_ps + 2 * BEAM_MAX);
    float* b_pnb = b_pb + 2 * BEAM_MAX;
    float* b_tot = b_pnb + 2 * BEAM_MAX;
    int* sel_src = (int*)(b_tot + 2 * BEAM_MAX);          // [BEAM_MAX] candidate index of each new slot
    int* b_state = sel_src + BEAM_MAX;                    // LM: automaton state after the entry's prefix, two generations
    float* b_w = (float*)(b_state + 2 * BEAM_MAX);        // LM: weight the prefix's last character paid (node_w)
    int* nstate = nullptr; float* nw = nullptr;
    if constexpr (LM) { nstate = a.node_state + (size_t)n * pool; nw = a.node_w + (size_t)n * pool; }
    __shared__ int s_cnt[4];
    __shared__ unsigned s_key;
    __shared__ int s_misc[4];

    // root: empty prefix, p_blank = 1, p_label = 0
    if (tid == 0) {
        b_node[0] = 0; b_last[0] = -1; b_ps[0] = -1; b_pb[0] = 0.f; b_pnb[0] = NEGINF; b_tot[0] = 0.f;
        npar[0] = -1; nlab[0] = -1; nslot[0] = 0;
        if constexpr (LM) { b_state[0] = 0; b_w[0] = 0.f; nstate[0] = 0; nw[0] = 0.f; }
        s_misc[0] = 1;        // beam size
        s_misc[1] = 1;        // nodes allocated
    }
    if constexpr (!WIDE) for (int i = tid; i < K * C; i += 256) table[i] = -1;
    __syncthreads();
    int gen = 0;
    for (int t = 0; t < Tn; ++t) {
        const int nb = s_misc[0];
        int* node = b_node + gen * BEAM_MAX; int* last = b_last + gen * BEAM_MAX; int* ps = b_ps + gen * BEAM_MAX;
        float* pb = b_pb + gen * BEAM_MAX; float* pnb = b_pnb + gen * BEAM_MAX; float* tot = b_tot + gen * BEAM_MAX;
        int* state = b_state + gen * BEAM_MAX; float* wlast = b_w + gen * BEAM_MAX;      // (LM only)
        // (a) log-softmax of the frame
        const float* row = a.act + ((size_t)t * a.N + n) * C;
        {
            float m = NEGINF;
            for (int k = tid; k < C; k += 256) m = fmaxf(m, row[k]);
            m = wave_max(m);
            if (lane == 0) ((float*)s_cnt)[wave] = m;
            __syncthreads();
            m = fmaxf(fmaxf(((float*)s_cnt)[0], ((float*)s_cnt)[1]), fmaxf(((float*)s_cnt)[2], ((float*)s_cnt)[3]));
            __syncthreads();
            float sum = 0.f;
            for (int k = tid; k < C; k += 256) sum += expf(row[k] - m);
            sum = wave_sum(sum);
            if (lane == 0) ((float*)s_cnt)[wave] = sum;
            __syncthreads();
            float lse = m + logf(((float*)s_cnt)[0] + ((float*)s_cnt)[1] + ((float*)s_cnt)[2] + ((float*)s_cnt)[3]);
            __syncthreads();
            if constexpr (NBEST) {
                const int ub = a.blank;                    // the caller's blank; internal index of class k (see the kernel's header)
                // (one loop: a loop per range, below and above the blank, exposes a second global-load latency per frame and measured slower)
                for (int k = tid; k < C; k += 256) lp[k < ub ? k : (k == ub ? C - 1 : k - 1)] = row[k] - lse;
            } else {
                for (int k = tid; k < C; k += 256) lp[k] = row[k] - lse;
            }
        }
        __syncthreads();
        // (a') wide kernel: S = the M non-blank classes with the largest lp, ascending.  M-th largest key by the bisection of step (d),
        // then an ordered compaction that takes everything above it and the first M - (number above) ties in class order.
        if constexpr (WIDE) {
            if (M == blank) {
                for (int j = tid; j < M; j += 256) sel_cls[j] = j;
            } else {
                unsigned lo = 0u, hi = 0xffffffffu;         // count(key >= 0) = C - 1 >= M
                while (lo < hi) {
                    const unsigned mid = lo + (unsigned)(((unsigned long long)hi - lo + 1ull) >> 1);
                    int cnt = 0;
                    for (int k = tid; k < blank; k += 256) cnt += (fkey(lp[k]) >= mid);
                    cnt = (int)wave_sum((float)cnt);
                    if (lane == 0) s_cnt[wave] = cnt;
                    __syncthreads();
                    cnt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
                    __syncthreads();
                    if (cnt >= M) lo = mid; else hi = mid - 1u;
                }
                const unsigned thr = lo;
                int above = 0;
                for (int k = tid; k < blank; k += 256) above += (fkey(lp[k]) > thr);
                above = (int)wave_sum((float)above);
                if (lane == 0) s_cnt[wave] = above;
                __syncthreads();
                const int quota = M - (s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);      // ties to take, >= 1
                if (wave == 0) {
                    int filled = 0, ties = 0;
                    for (int base = 0; base < blank; base += 64) {
                        const int k = base + lane;
                        const unsigned key = (k < blank) ? fkey(lp[k]) : 0u;
                        const bool eq = (k < blank) && key == thr;
                        const unsigned long long below = (1ull << lane) - 1ull;
                        const unsigned long long eqmask = __ballot(eq);
                        const bool take = (k < blank) && (key > thr || (eq && ties + __popcll(eqmask & below) < quota));
                        const unsigned long long mask = __ballot(take);
                        const int posn = filled + __popcll(mask & below);
                        if (take && posn < M) sel_cls[posn] = k;
                        filled += __popcll(mask);
                        ties += __popcll(eqmask);
                    }
                }
            }
            __syncthreads();
        }
        // (b) leaves stay in the beam with updated probabilities; cand[s] = new total
        float my_npb = NEGINF, my_npnb = NEGINF;
        if (tid < nb) {
            const int s = tid;
            float nl = NEGINF;
            if (last[s] >= 0) {
                nl = pnb[s];
                const int p = ps[s];
                if constexpr (LM) {
                    if (p >= 0) nl = blse(nl, ((last[s] == last[p]) ? pb[p] : tot[p]) + wlast[s]);     // the parent's mass pays this character's weight
                } else {
                    if (p >= 0) nl = blse(nl, (last[s] == last[p]) ? pb[p] : tot[p]);
                }
                if (nl != NEGINF) nl += lp[last[s]];
            }
            my_npnb = nl;
            my_npb = tot[s] + lp[blank];
            cand[s] = blse(my_npb, my_npnb);
        }
        // (c) children that are not in the beam: cand[nb + b*C + c]  (wide: cand[nb + b*M + j] for class S[j])
        if constexpr (!WIDE) {
            for (int i = tid; i < nb * C; i += 256) {
                const int b = i / C, c = i - b * C;
                float v = NEGINF;
                if (c != blank && table[b * C + c] < 0) {
                    const float prev = (c == last[b]) ? pb[b] : tot[b];
                    if constexpr (LM) {
                        // state[b] < num_states and the caller's class id < C: inside the tables whatever they hold
                        const size_t e = (size_t)state[b] * C + (c < a.blank ? c : c + 1);
                        const float w = a.lm_weight[e];
                        const unsigned nx = (unsigned)a.lm_next[e];
                        if (prev != NEGINF && lm_finite(w) && nx < (unsigned)a.num_states) v = prev + lp[c] + w;
                    } else {
                        if (prev != NEGINF) v = prev + lp[c];
                    }
                }
                cand[nb + i] = v;
            }
            __syncthreads();
        } else {
            for (int i = tid; i < nb * M; i += 256) {
                const int b = i / M, c = sel_cls[i - b * M];
                const float prev = (c == last[b]) ? pb[b] : tot[b];
                if constexpr (LM) {
                    float v = NEGINF, w; int nx;
                    if (prev != NEGINF && sparse_step(a, state[b], c < a.blank ? c : c + 1, w, nx)) v = prev + lp[c] + w;
                    cand[nb + i] = v;
                } else {
                    cand[nb + i] = (prev != NEGINF) ? prev + lp[c] : NEGINF;
                }
            }
            __syncthreads();
            // a beam entry whose parent is in the beam cancels the candidate (parent, own label), if its label is in S
            if (tid < nb && ps[tid] >= 0) {
                const int c = last[tid];
                int l = 0, r = M;                              // first j with S[j] >= c
                while (l < r) { const int mid = (l + r) >> 1; if (sel_cls[mid] < c) l = mid + 1; else r = mid; }
                if (l < M && sel_cls[l] == c) cand[nb + ps[tid] * M + l] = NEGINF;
            }
            __syncthreads();
        }
        // (d) K-th largest candidate: bisection over the integer image
        const int ncand = nb + nb * M;
        unsigned lo = 0u, hi = 0xffffffffu;                // invariant: count(key >= lo) >= K or lo == 0
        {
            int finite = 0;
            for (int i = tid; i < ncand; i += 256) finite += (cand[i] != NEGINF);
            finite = (int)wave_sum((float)finite);
            if (lane == 0) s_cnt[wave] = finite;
            __syncthreads();
            finite = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            __syncthreads();
            if (finite <= K) { lo = fkey(NEGINF) + 1u; hi = lo; }      // keep every finite candidate
        }
        while (lo < hi) {                                   // find the largest key `lo` with count(key >= lo) >= K
            const unsigned mid = lo + (unsigned)(((unsigned long long)hi - lo + 1ull) >> 1);
            int cnt = 0;
            for (int i = tid; i < ncand; i += 256) cnt += (fkey(cand[i]) >= mid);
            cnt = (int)wave_sum((float)cnt);
            if (lane == 0) s_cnt[wave] = cnt;
            __syncthreads();
            cnt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            __syncthreads();
            if (cnt >= K) lo = mid; else hi = mid - 1u;
        }
        const unsigned thr = lo;
        // (e) ordered compaction: everything above the threshold, then ties in index order until the beam is full
        if (tid == 0) { s_misc[2] = 0; }
        __syncthreads();
        if (wave == 0) {
            int filled = 0;
            for (int pass = 0; pass < 2; ++pass) {
                for (int base = 0; base < ncand; base += 64) {
                    const int i = base + lane;
                    bool take = false;
                    if (i < ncand) {
                        const unsigned k = fkey(cand[i]);
                        take = (pass == 0) ? (k > thr) : (k == thr && cand[i] != NEGINF);
                    }
                    unsigned long long mask = __ballot(take);
                    int posn = filled + __popcll(mask & ((1ull << lane) - 1ull));
                    if (take && posn < K) sel_src[posn] = i;
                    filled = min(K, filled + __popcll(mask));
                }
            }
            if (lane == 0) s_misc[2] = filled;
        }
        __syncthreads();
        const int nnew = s_misc[2];
        // (f) next generation
        const int g2 = gen ^ 1;
        int* node2 = b_node + g2 * BEAM_MAX; int* last2 = b_last + g2 * BEAM_MAX; int* ps2 = b_ps + g2 * BEAM_MAX;
        float* pb2 = b_pb + g2 * BEAM_MAX; float* pnb2 = b_pnb + g2 * BEAM_MAX; float* tot2 = b_tot + g2 * BEAM_MAX;
        // stash the updated leaf probabilities where the compaction can find them (old arrays are re-read below first)
        float* upd_pb = cand;          // reuse cand[0..nb) AFTER the totals were consumed? totals are still needed -> use table space? no:
        __syncthreads();
        // leaves' new (p_blank, p_label) live in registers of thread s; publish them through the dead half of the beam arrays
        if (tid < nb) { pb2[tid] = my_npb; pnb2[tid] = my_npnb; }     // temporarily indexed by OLD slot
        float r_pb = NEGINF, r_pnb = NEGINF, r_tot = NEGINF; int r_node = -1, r_last = -1, r_src = -1;
        int r_state = 0; float r_w = 0.f;
        if (tid < nnew) { r_src = sel_src[tid]; r_tot = cand[r_src]; }
        __syncthreads();
        // One node per prefix: a child that enters the beam may be a prefix that was in it before (see the header).  Its node is found by
        // one pass over the pool: node `id` is such a child iff its parent sits in the (old) beam at slot b and candidate (b, nlab[id])
        // was selected.  cand and sel_src are dead by now: cand becomes the map candidate -> new slot, sel_src the node each new slot reuses.
        int* cslot = (int*)cand;
        for (int i = nb + tid; i < ncand; i += 256) cslot[i] = -1;
        __syncthreads();
        if (tid < nnew) { sel_src[tid] = -1; if (r_src >= nb) cslot[r_src] = tid; }
        __syncthreads();
        const int nalloc = s_misc[1];
        for (int id = 1 + tid; id < nalloc; id += 256) {
            const int b = nslot[npar[id]];                  // still the old generation's slots
            if (b < 0) continue;
            int j = nlab[id];
            if constexpr (WIDE) {
                const int c = j;
                int l = 0, r = M;                            // first j with S[j] >= c
                while (l < r) { const int mid = (l + r) >> 1; if (sel_cls[mid] < c) l = mid + 1; else r = mid; }
                j = (l < M && sel_cls[l] == c) ? l : -1;
            }
            if (j < 0) continue;
            const int s = cslot[nb + b * M + j];
            if (s >= 0) sel_src[s] = id;
        }
        __syncthreads();
        if (tid < nb) nslot[node[tid]] = -1;                           // everything is out of the beam until re-registered
        __syncthreads();
        if (tid < nnew) {
            const int i = r_src;
            if (i < nb) {                                   // surviving leaf
                r_node = node[i]; r_last = last[i]; r_pb = pb2[i]; r_pnb = pnb2[i];
                if constexpr (LM) { r_state = state[i]; r_w = wlast[i]; }
            } else {                                        // child of leaf b with label c: back on its old node, or new
                const int b = (i - nb) / M, c = WIDE ? sel_cls[(i - nb) - b * M] : (i - nb) - b * M;
                int id = sel_src[tid];
                if (id < 0) {
                    id = atomicAdd(&s_misc[1], 1);
                    npar[id] = node[b]; nlab[id] = (short)c;
                    if constexpr (LM && WIDE) {             // admitted, so step (c) found this transition: the same walk, the same (w, next)
                        if (!sparse_step(a, state[b], c < a.blank ? c : c + 1, r_w, r_state)) { r_state = 0; r_w = NEGINF; }      // (never taken)
                        nstate[id] = r_state; nw[id] = r_w;
                    } else if constexpr (LM) {              // admitted, so step (c) found the weight finite and the next state in range
                        const size_t e = (size_t)state[b] * C + (c < a.blank ? c : c + 1);
                        r_state = a.lm_next[e]; r_w = a.lm_weight[e];
                        nstate[id] = r_state; nw[id] = r_w;
                    }
                } else if constexpr (LM) {                  // back on its old node: the state and the weight it was given then
                    r_state = nstate[id]; r_w = nw[id];
                }
                r_node = id; r_last = c; r_pb = NEGINF; r_pnb = r_tot;
            }
        }
        __syncthreads();
        if (tid < nnew) {
            node2[tid] = r_node; last2[tid] = r_last; pb2[tid] = r_pb; pnb2[tid] = r_pnb; tot2[tid] = r_tot;
            nslot[r_node] = tid;
            if constexpr (LM) { (b_state + g2 * BEAM_MAX)[tid] = r_state; (b_w + g2 * BEAM_MAX)[tid] = r_w; }
        }
        if constexpr (!WIDE) for (int i = tid; i < K * C; i += 256) table[i] = -1;
        __syncthreads();
        if (tid < nnew) {
            const int par = npar[node2[tid]];
            const int p = (par >= 0) ? nslot[par] : -1;
            ps2[tid] = p;
            if constexpr (!WIDE) if (p >= 0) table[p * C + last2[tid]] = (short)tid;
        }
        if (tid == 0) s_misc[0] = nnew;
        __syncthreads();
        gen = g2;
        (void)upd_pb;
    }
    if constexpr (NBEST) {
        // ---- the top_paths best leaves under the total order (total descending, then lower slot), ranked by counting: thread s counts the
        // entries ahead of it.  -inf totals are never returned (they rank behind every finite one, so they do not disturb the counts).
        const int nb = s_misc[0], P = a.top_paths, ub = a.blank;
        const float* tot = b_tot + gen * BEAM_MAX; const int* node = b_node + gen * BEAM_MAX;
        if constexpr (LM) {                                  // ranked by total + final[state]; a state that may not end the string is -inf
            float* key = (float*)smem_raw + ((C + 3) & ~3);     // cand is dead
            if (tid < nb) {
                const float f = a.lm_final[(b_state + gen * BEAM_MAX)[tid]];
                key[tid] = lm_finite(f) ? tot[tid] + f : NEGINF;
            }
            __syncthreads();
            tot = key;
        }
        int valid = 0;
        for (int s = 0; s < nb; ++s) valid += (tot[s] != NEGINF);
        const int cnt = min(valid, P);
        if (tid < nb && tot[tid] != NEGINF) {
            const float mine = tot[tid];
            int rank = 0;
            for (int s = 0; s < nb; ++s) rank += (tot[s] > mine || (tot[s] == mine && s < tid));
            if (rank < P) {                                  // this thread walks its own path root-ward
                int* o = a.out + ((size_t)n * P + rank) * a.T;
                int len = 0;
                float lmw = 0.f;                              // LM: W(P), the weights along the path
                for (int id = node[tid]; id > 0; id = npar[id]) {                                                                 // reversed
                    const int c = nlab[id]; o[len++] = (c < ub) ? c : c + 1;
                    if constexpr (LM) lmw += nw[id];
                }
                for (int i = 0; i < len / 2; ++i) { int tmp = o[i]; o[i] = o[len - 1 - i]; o[len - 1 - i] = tmp; }
                if (a.merge_repeated) {
                    int w = 0;
                    for (int i = 0; i < len; ++i) if (i == 0 || o[i] != o[i - 1]) o[w++] = o[i];
                    len = w;
                }
                for (int i = len; i < a.T; ++i) o[i] = a.pad_value;
                a.out_len[(size_t)n * P + rank] = len;
                a.neg_log_prob[(size_t)n * P + rank] = -mine;
                if constexpr (LM) a.lm_score[(size_t)n * P + rank] = lmw + a.lm_final[(b_state + gen * BEAM_MAX)[tid]];
            }
        }
        if (tid >= cnt && tid < P) {                         // no path for these slots (P <= 128 < 256 threads)
            int* o = a.out + ((size_t)n * P + tid) * a.T;
            for (int i = 0; i < a.T; ++i) o[i] = a.pad_value;
            a.out_len[(size_t)n * P + tid] = -1;
            a.neg_log_prob[(size_t)n * P + tid] = INFINITY;
            if constexpr (LM) a.lm_score[(size_t)n * P + tid] = NEGINF;
        }
        if (tid == 0) a.count[n] = cnt;
        return;
    }
    // ---- best leaf, label sequence (root-ward walk), merge_repeated, output
    if (tid == 0) {
        const int nb = s_misc[0];
        float* tot = b_tot + gen * BEAM_MAX; int* node = b_node + gen * BEAM_MAX;
        int best = 0;
        for (int s = 1; s < nb; ++s) if (tot[s] > tot[best]) best = s;
        int* o = a.out + (size_t)n * a.T;
        int len = 0;
        for (int id = node[best]; id > 0; id = npar[id]) o[len++] = nlab[id];      // reversed
        for (int i = 0; i < len / 2; ++i) { int tmp = o[i]; o[i] = o[len - 1 - i]; o[len - 1 - i] = tmp; }
        if (a.merge_repeated) {
            int w = 0;
            for (int i = 0; i < len; ++i) if (i == 0 || o[i] != o[i - 1]) o[w++] = o[i];
            len = w;
        }
        for (int i = len; i < a.T; ++i) o[i] = a.pad_value;
        a.out_len[n] = len;
        if (a.neg_log_prob) a.neg_log_prob[n] = -tot[best];
    }
}

static size_t beam_lds_bytes(int C, int K) {
    const size_t kc = (size_t)K * (size_t)C;
    size_t b = (size_t)(((size_t)C + 3) & ~(size_t)3) * 4 + ((size_t)K + kc) * 4 + ((kc + 1) & ~(size_t)1) * 2 + (size_t)BEAM_MAX * 2 * 6 * 4 +
               (size_t)BEAM_MAX * 4;
    return (b + 15) & ~(size_t)15;
}
static size_t beam_wide_lds_bytes(int C, int K) {
    const size_t M = (size_t)((K + 1 < C - 1) ? K + 1 : C - 1);
    size_t b = (size_t)((C + 3) & ~3) * 4 + ((size_t)K + (size_t)K * M) * 4 + M * 4 + (size_t)BEAM_MAX * 2 * 6 * 4 + (size_t)BEAM_MAX * 4;
    return (b + 15) & ~(size_t)15;
}

static size_t beam_lm_lds_bytes(int C, int K) {          // the table kernel's, and b_state / b_w: two more [2][BEAM_MAX] arrays
    return beam_lds_bytes(C, K) + (size_t)BEAM_MAX * 2 * 2 * 4;
}
#define BEAM_LM_MAX_STATES (1 << 20)

static int g_beam_engine = 0;
extern "C" int ocr_set_beam_engine(int engine) {       // A/B + test knob: 0 = table kernel where it fits, 2 = wide kernel wherever it covers
    if (engine != 0 && engine != 2) return OCR_ERR_INVALID;
    g_beam_engine = engine;
    return OCR_OK;
}
// 0 refused, 1 table kernel, 2 wide kernel: what ocr_ctc_beam_decode launches by
extern "C" int ocr_ctc_beam_kernel_choice(int alphabet_size, int beam_width) {
    if (alphabet_size < 2 || beam_width <= 0 || beam_width > BEAM_MAX) return 0;
    const bool table = beam_lds_bytes(alphabet_size, beam_width) <= BEAM_LDS_LIMIT;
    const bool wide = alphabet_size <= BEAM_WIDE_MAX_C && beam_wide_lds_bytes(alphabet_size, beam_width) <= BEAM_LDS_LIMIT;
    if (g_beam_engine == 2 && wide) return 2;
    return table ? 1 : (wide ? 2 : 0);
}

extern "C" int ocr_ctc_beam_workspace_size(int alphabet_size, int minibatch, int max_time, int beam_width, size_t* bytes) {
    if (!bytes || alphabet_size < 2 || minibatch <= 0 || max_time <= 0 || beam_width <= 0 || beam_width > BEAM_MAX)
        return OCR_ERR_INVALID;
    if (ocr_ctc_beam_kernel_choice(alphabet_size, beam_width) == 0) return OCR_ERR_INVALID;
    size_t pool = (size_t)max_time * beam_width + 2;
    *bytes = (size_t)minibatch * pool * (sizeof(int) * 2 + sizeof(short));
    *bytes = (*bytes + 255) & ~(size_t)255;
    return OCR_OK;
}

template <bool NBEST>
static int beam_launch(const BeamArgs& a, hipStream_t stream) {
    if (ocr_ctc_beam_kernel_choice(a.C, a.K) == 2) {
        const size_t lds = beam_wide_lds_bytes(a.C, a.K);
        if (ocr_allow_lds<ctc_beam_kernel<true, NBEST>>((int)lds) != hipSuccess) return OCR_ERR_EXEC;
        ctc_beam_kernel<true, NBEST><<<a.N, 256, lds, stream>>>(a);
    } else {
        const size_t lds = beam_lds_bytes(a.C, a.K);
        if (ocr_allow_lds<ctc_beam_kernel<false, NBEST>>((int)lds) != hipSuccess) return OCR_ERR_EXEC;
        ctc_beam_kernel<false, NBEST><<<a.N, 256, lds, stream>>>(a);
    }
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
static void beam_workspace(BeamArgs& a, void* workspace) {
    const size_t pool = (size_t)a.T * a.K + 2;
    a.node_parent = (int*)workspace;
    a.node_slot = a.node_parent + (size_t)a.N * pool;
    a.node_label = (short*)(a.node_slot + (size_t)a.N * pool);
}

extern "C" int ocr_ctc_beam_decode(const float* activations, const int* input_lengths, int alphabet_size, int minibatch,
                                   int max_time, int beam_width, int merge_repeated, int pad_value, int* decoded,
                                   int* decoded_lengths, float* neg_log_prob, void* workspace, size_t workspace_bytes,
                                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    size_t need = 0;
    if (!activations || !input_lengths || !decoded || !decoded_lengths || !workspace) return OCR_ERR_INVALID;
    if (ocr_ctc_beam_workspace_size(alphabet_size, minibatch, max_time, beam_width, &need) != OCR_OK || workspace_bytes < need)
        return OCR_ERR_INVALID;
    BeamArgs a = {activations, input_lengths, max_time, minibatch, alphabet_size, beam_width, merge_repeated, pad_value,
                  decoded, decoded_lengths, neg_log_prob, nullptr, nullptr, nullptr, alphabet_size - 1, 1, nullptr};
    beam_workspace(a, workspace);
    return beam_launch<false>(a, stream);
}

// The top_paths best prefixes per sample, best first, for any blank class (see the kernel's header).  decoded [N, top_paths, T],
// decoded_lengths / neg_log_prob [N, top_paths], count [N]; slots at and beyond count[n] hold pad_value / -1 / +inf.
extern "C" int ocr_ctc_beam_decode_nbest(const float* activations, const int* input_lengths, int alphabet_size, int minibatch,
                                         int max_time, int beam_width, int top_paths, int blank, int merge_repeated, int pad_value,
                                         int* decoded, int* decoded_lengths, float* neg_log_prob, int* count, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    size_t need = 0;
    if (!activations || !input_lengths || !decoded || !decoded_lengths || !neg_log_prob || !count || !workspace) return OCR_ERR_INVALID;
    if (ocr_ctc_beam_workspace_size(alphabet_size, minibatch, max_time, beam_width, &need) != OCR_OK || workspace_bytes < need)
        return OCR_ERR_INVALID;
    if (top_paths < 1 || top_paths > beam_width || blank < 0 || blank >= alphabet_size) return OCR_ERR_INVALID;
    BeamArgs a = {activations, input_lengths, max_time, minibatch, alphabet_size, beam_width, merge_repeated, pad_value,
                  decoded, decoded_lengths, neg_log_prob, nullptr, nullptr, nullptr, blank, top_paths, count};
    beam_workspace(a, workspace);
    return beam_launch<true>(a, stream);
}

// ---- the search fused with a label automaton (LM = true; the table kernel only)
extern "C" int ocr_ctc_beam_lm_supported(int alphabet_size, int beam_width, int num_states) {
    if (alphabet_size < 2 || beam_width < 1 || beam_width > BEAM_MAX || num_states < 1 || num_states > BEAM_LM_MAX_STATES) return 0;
    return beam_lm_lds_bytes(alphabet_size, beam_width) <= BEAM_LDS_LIMIT ? 1 : 0;
}
// node_parent, node_slot, node_state (int), node_w (float), node_label (short) per pool entry
extern "C" int ocr_ctc_beam_lm_workspace_size(int alphabet_size, int minibatch, int max_time, int beam_width, size_t* bytes) {
    if (!bytes || minibatch <= 0 || max_time <= 0 || !ocr_ctc_beam_lm_supported(alphabet_size, beam_width, 1)) return OCR_ERR_INVALID;
    const size_t pool = (size_t)max_time * beam_width + 2;
    *bytes = (size_t)minibatch * pool * (sizeof(int) * 3 + sizeof(float) + sizeof(short));
    *bytes = (*bytes + 255) & ~(size_t)255;
    return OCR_OK;
}
// The top_paths best prefixes under total(P) + final[state(P)], best first; neg_log_prob = -(that sum), lm_score = W(P) + final, so
// -neg_log_prob - lm_score is the beam's acoustic log-probability.  Outputs as ocr_ctc_beam_decode_nbest's, lm_score -inf beyond count[n].
extern "C" int ocr_ctc_beam_decode_lm(const float* activations, const int* input_lengths, int alphabet_size, int minibatch, int max_time,
                                      int beam_width, int top_paths, int blank, int pad_value, const int* lm_next, const float* lm_weight,
                                      const float* lm_final, int num_states, int* decoded, int* decoded_lengths, float* neg_log_prob,
                                      float* lm_score, int* count, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    size_t need = 0;
    if (!activations || !input_lengths || !lm_next || !lm_weight || !lm_final || !decoded || !decoded_lengths || !neg_log_prob || !lm_score ||
        !count || !workspace)
        return OCR_ERR_INVALID;
    if (!ocr_ctc_beam_lm_supported(alphabet_size, beam_width, num_states)) return OCR_ERR_INVALID;
    if (ocr_ctc_beam_lm_workspace_size(alphabet_size, minibatch, max_time, beam_width, &need) != OCR_OK || workspace_bytes < need)
        return OCR_ERR_INVALID;
    if (top_paths < 1 || top_paths > beam_width || blank < 0 || blank >= alphabet_size) return OCR_ERR_INVALID;
    BeamLmArgs a;
    (BeamArgs&)a = {activations, input_lengths, max_time, minibatch, alphabet_size, beam_width, 0, pad_value,
                    decoded, decoded_lengths, neg_log_prob, nullptr, nullptr, nullptr, blank, top_paths, count};
    const size_t pool = (size_t)max_time * beam_width + 2, all = (size_t)minibatch * pool;
    a.node_parent = (int*)workspace;
    a.node_slot = a.node_parent + all;
    a.node_state = a.node_slot + all;
    a.node_w = (float*)(a.node_state + all);
    a.node_label = (short*)(a.node_w + all);
    a.lm_next = lm_next; a.lm_weight = lm_weight; a.lm_final = lm_final; a.num_states = num_states; a.lm_score = lm_score;
    const size_t lds = beam_lm_lds_bytes(alphabet_size, beam_width);
    if (ocr_allow_lds<ctc_beam_kernel<false, true, true>>((int)lds) != hipSuccess) return OCR_ERR_EXEC;
    ctc_beam_kernel<false, true, true><<<minibatch, 256, lds, stream>>>(a);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}

// ---- the search fused with a sparse back-off automaton (LM = true on the wide kernel, whatever ocr_set_beam_engine says)
#define BEAM_SPARSE_MAX_STATES (1 << 24)
#define BEAM_SPARSE_MAX_ARCS (1 << 28)
static size_t beam_sparse_lds_bytes(int C, int K, int cutoff) {      // the wide kernel's with M = min(cutoff, C - 1), and b_state / b_w
    const size_t M = (size_t)((cutoff < C - 1) ? cutoff : C - 1);
    size_t b = (size_t)((C + 3) & ~3) * 4 + ((size_t)K + (size_t)K * M) * 4 + M * 4 + (size_t)BEAM_MAX * 2 * 6 * 4 + (size_t)BEAM_MAX * 4;
    return ((b + 15) & ~(size_t)15) + (size_t)BEAM_MAX * 2 * 2 * 4;
}
extern "C" int ocr_ctc_beam_lm_sparse_supported(int alphabet_size, int beam_width, int cutoff, int num_states, int num_arcs) {
    if (alphabet_size < 2 || alphabet_size > BEAM_WIDE_MAX_C || beam_width < 1 || beam_width > BEAM_MAX) return 0;
    if (cutoff < 1 || cutoff > beam_width + 1) return 0;
    if (num_states < 1 || num_states > BEAM_SPARSE_MAX_STATES || num_arcs < 0 || num_arcs > BEAM_SPARSE_MAX_ARCS) return 0;
    return beam_sparse_lds_bytes(alphabet_size, beam_width, cutoff) <= BEAM_LDS_LIMIT ? 1 : 0;
}
// per pool entry what ocr_ctc_beam_lm_workspace_size counts: node_parent, node_slot, node_state (int), node_w (float), node_label (short)
extern "C" int ocr_ctc_beam_lm_sparse_workspace_size(int alphabet_size, int minibatch, int max_time, int beam_width, size_t* bytes) {
    if (!bytes || minibatch <= 0 || max_time <= 0 || !ocr_ctc_beam_lm_sparse_supported(alphabet_size, beam_width, 1, 1, 0)) return OCR_ERR_INVALID;
    const size_t pool = (size_t)max_time * beam_width + 2;
    *bytes = (size_t)minibatch * pool * (sizeof(int) * 3 + sizeof(float) + sizeof(short));
    *bytes = (*bytes + 255) & ~(size_t)255;
    return OCR_OK;
}
// Outputs and refusals as ocr_ctc_beam_decode_lm's; new children of a frame come from its min(cutoff, C - 1) likeliest non-blank classes.
extern "C" int ocr_ctc_beam_decode_lm_sparse(const float* activations, const int* input_lengths, int alphabet_size, int minibatch, int max_time,
                                             int beam_width, int cutoff, int top_paths, int blank, int pad_value, const int* arc_begin,
                                             const int* arc_label, const int* arc_next, const float* arc_weight, const int* backoff,
                                             const float* backoff_weight, const float* lm_final, int num_states, int num_arcs, int* decoded,
                                             int* decoded_lengths, float* neg_log_prob, float* lm_score, int* count, void* workspace,
                                             size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    size_t need = 0;
    if (!activations || !input_lengths || !arc_begin || !arc_label || !arc_next || !arc_weight || !backoff || !backoff_weight || !lm_final ||
        !decoded || !decoded_lengths || !neg_log_prob || !lm_score || !count || !workspace)
        return OCR_ERR_INVALID;
    if (!ocr_ctc_beam_lm_sparse_supported(alphabet_size, beam_width, cutoff, num_states, num_arcs)) return OCR_ERR_INVALID;
    if (ocr_ctc_beam_lm_sparse_workspace_size(alphabet_size, minibatch, max_time, beam_width, &need) != OCR_OK || workspace_bytes < need)
        return OCR_ERR_INVALID;
    if (top_paths < 1 || top_paths > beam_width || blank < 0 || blank >= alphabet_size) return OCR_ERR_INVALID;
    BeamSparseArgs a;
    (BeamArgs&)a = {activations, input_lengths, max_time, minibatch, alphabet_size, beam_width, 0, pad_value,
                    decoded, decoded_lengths, neg_log_prob, nullptr, nullptr, nullptr, blank, top_paths, count};
    const size_t pool = (size_t)max_time * beam_width + 2, all = (size_t)minibatch * pool;
    a.node_parent = (int*)workspace;
    a.node_slot = a.node_parent + all;
    a.node_state = a.node_slot + all;
    a.node_w = (float*)(a.node_state + all);
    a.node_label = (short*)(a.node_w + all);
    a.arc_begin = arc_begin; a.arc_label = arc_label; a.arc_next = arc_next; a.arc_weight = arc_weight;
    a.backoff = backoff; a.backoff_weight = backoff_weight; a.lm_final = lm_final;
    a.num_states = num_states; a.num_arcs = num_arcs; a.cutoff = cutoff; a.lm_score = lm_score;
    const size_t lds = beam_sparse_lds_bytes(alphabet_size, beam_width, cutoff);
    if (ocr_allow_lds<ctc_beam_kernel<true, true, true>>((int)lds) != hipSuccess) return OCR_ERR_EXEC;
    ctc_beam_kernel<true, true, true><<<minibatch, 256, lds, stream>>>(a);
    OCR_CHECK_LAUNCH();
    return OCR_OK;
}
