/* libocrhip — C ABI of the MI355X (gfx950) CRNN-OCR hot path.
 *
 * Conventions (the same ones baidu warp-ctc's `compute_ctc_loss` uses, which is the only FFI the reference
 * itself crosses — /root/reference/lib/networks/network.py:6,653-654):
 *   - every pointer is a caller-owned DEVICE pointer (HBM) unless stated otherwise; the library keeps no state,
 *     allocates nothing and never synchronises; all work is enqueued on `stream` (a hipStream_t passed as void*);
 *   - return value is an int status: 0 ok, 1 memory-op failed, 2 invalid argument, 3 launch failed
 *     (warp-ctc's ctcStatus_t numbering); no exceptions, no torch types;
 *   - "bf16" buffers hold raw bfloat16 bits (uint16_t); activations use the reference layout [N, W, H, C]
 *     (image width W = time is TF's "height" axis, the 32-pixel feature axis H is TF's "width": gen.py:63-64).
 *
 * Each entry point cites the reference line whose computation it replaces.
 */
#ifndef OCR_HIP_H
#define OCR_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { OCR_STATUS_OK = 0, OCR_STATUS_MEMOPS = 1, OCR_STATUS_INVALID = 2, OCR_STATUS_EXEC = 3 };

/* epilogue flags of the GEMM / implicit-GEMM convolution engine */
enum {
    OCR_EPI_BIAS = 1, OCR_EPI_RELU = 2, OCR_EPI_OUT_F32 = 4, /* 8 reserved (split-K atomics, set internally) */
    OCR_EPI_MASK = 16, OCR_EPI_ROWSWAP = 32, OCR_EPI_ACCUM = 64
};

const char* ocr_status_string(int status);           /* warp-ctc: ctcGetStatusString */
int ocr_abi_version(void);
/* first 16 hex digits of sha256 over the sources this library was built from (csrc/Makefile; "-exp" appended by the experiments
 * flavour): profiles are pinned to it, and lstm_ctc_ocr_amd._native.source_build_id() recomputes it from the tree to detect a stale .so */
const char* ocr_build_id(void);

/* ---- CTC (replaces warpctc_tensorflow.ctc, network.py:653-654; warp-ctc get_workspace_size/compute_ctc_loss) */
/* ctc.hip: the general one-wave kernel and the fast kernel (S = 2L+1 <= 64, tables in LDS); every CTC kernel derives its sample's label
 * offset itself, no scan launch */
int ocr_ctc_workspace_size(int max_label_len, int max_time, int minibatch, size_t* bytes);
/* activations/gradients: f32 [max_time, minibatch, alphabet_size], unnormalised; gradients may be NULL (score only).
 * flat_labels / label_lengths / input_lengths are DEVICE int32 arrays (warp-ctc's GPU path takes them from the host;
 * keeping them in HBM removes the per-step host sync of train.py:130).  costs: f32 [minibatch]. */
int ocr_ctc_loss(const float* activations, float* gradients, const int* flat_labels, const int* label_lengths,
                 const int* input_lengths, int alphabet_size, int minibatch, int max_time, int max_label_len,
                 int blank_label, float* costs, void* workspace, void* stream);
/* training form: one launch producing costs and scale * gradient as bf16 [minibatch][max_time][alphabet] (what the backward
 * GEMMs read); label offsets computed in-kernel.  ocr_ctc_train_supported() == 0 -> use ocr_ctc_loss + ocr_tnc_to_ntc_bf16 */
/* diagnostic: device int64[5] receiving 100 MHz wall-clock stamps at the phase boundaries of sample 0 of the fast kernel (NULL = off);
 * the stamps are compiled only into the experiments build (make EXPERIMENTS=1), the product library stores the pointer and never reads it */
int ocr_ctc_debug(void* dbg);
int ocr_ctc_train_supported(int alphabet_size, int max_time, int max_label_len);
int ocr_ctc_loss_train(const float* activations, void* grad_ntc_bf16, float scale, const int* flat_labels,
                       const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch, int max_time,
                       int max_label_len, int blank_label, float* costs, void* stream);
int ocr_set_ctc_engine(int fast);   /* 1 (default): 4-wave LDS-resident kernel where it fits; 0: one-wave general kernel */
/* ctc_long.hip.  Long labels, 1 <= max_label_len <= 255 (S = 2L+1 <= 511): one launch, one 16-wave workgroup per sample, 2 / 4 / 8 extended-label slots
 * per lane.  Same semantics as ocr_ctc_loss; label offsets computed in-kernel.  Writes the f32 [T][N][C] gradient, the bf16 [N][T][C]
 * gradient multiplied by `scale`, both, or neither (score only).  The [T][S] tables live in LDS when they fit and in `workspace`
 * otherwise: ocr_ctc_long_placement = 0 not covered, 1 LDS, 2 workspace (arithmetic only); ocr_ctc_long_workspace_size gives 0 bytes for
 * placement 1, and `workspace` may then be NULL.  ocr_ctc_long_supported = placement != 0 and the device grants the LDS. */
int ocr_ctc_long_placement(int alphabet_size, int max_time, int max_label_len);
int ocr_ctc_long_supported(int alphabet_size, int max_time, int max_label_len);
int ocr_ctc_long_workspace_size(int alphabet_size, int max_label_len, int max_time, int minibatch, size_t* bytes);
int ocr_ctc_loss_long(const float* activations, float* gradients /* f32 [T][N][C] or NULL */,
                      void* grad_ntc_bf16 /* [N][T][C] or NULL */, float scale,
                      const int* flat_labels, const int* label_lengths, const int* input_lengths,
                      int alphabet_size, int minibatch, int max_time, int max_label_len, int blank_label,
                      float* costs, void* workspace, size_t workspace_bytes, void* stream);
/* wide alphabets, 1 <= alphabet_size <= 16384 and 1 <= max_label_len <= 255: the shapes beyond the LDS class accumulators of the two forms
 * above.  Two launches on `stream`: one workgroup per logit row (softmax * scale into the gradients, log-probabilities of the label's slots
 * into `workspace`), then one workgroup per sample (alpha / beta, costs, and the at most 2L+1 gradient elements per frame that are not plain
 * softmax).  Parameters, outputs and semantics as ocr_ctc_loss_long; `workspace` is always needed (ocr_ctc_wide_workspace_size bytes:
 * three [T][64 * slots-per-lane] float tables per sample).  ocr_ctc_wide_supported is arithmetic only and works without a GPU.
 * OCR_STATUS_INVALID, with nothing launched, for a NULL operand (the two gradients excepted), a blank outside [0, alphabet_size), a shape
 * ocr_ctc_wide_supported refuses, or a workspace that is short. */
int ocr_ctc_wide_supported(int alphabet_size, int max_time, int max_label_len);
int ocr_ctc_wide_workspace_size(int alphabet_size, int max_label_len, int max_time, int minibatch, size_t* bytes);
int ocr_ctc_loss_wide(const float* activations, float* gradients /* f32 [T][N][C] or NULL */,
                      void* grad_ntc_bf16 /* [N][T][C] or NULL */, float scale,
                      const int* flat_labels, const int* label_lengths, const int* input_lengths,
                      int alphabet_size, int minibatch, int max_time, int max_label_len, int blank_label,
                      float* costs, void* workspace, size_t workspace_bytes, void* stream);
/* lexicon scoring: costs[n][k] = -log p(candidate k | logits of sample n) for num_candidates strings against ONE set of logits (no copy per
 * candidate), 1 <= alphabet_size <= 16384, max_time >= 1, 0 <= max_label_len <= 255, 1 <= num_candidates <= 65536 (ocr_ctc_score_supported:
 * arithmetic only, works without a GPU).  Three launches on `stream`: the log-sum-exp of every logit row a sample owns into `workspace`
 * (ocr_ctc_score_workspace_size bytes: a float per row), one wave per (sample, candidate) running the alpha recursion in registers, one
 * workgroup per sample for the arg-min and the normaliser.
 *   cand_labels  : int32 [num_candidates][max_label_len], dense; cand_lengths: int32 [num_candidates].  sample_stride = 0: one lexicon shared
 *                  by every sample.  sample_stride = num_candidates: a lexicon per sample, labels [minibatch][num_candidates][max_label_len],
 *                  lengths [minibatch][num_candidates].  Words beyond a candidate's length are never read.
 *   costs        : f32 [minibatch][num_candidates].  +inf, never 0, for a candidate that cannot be emitted: input length <= 0, length + repeats
 *                  above the input length, a length outside [0, max_label_len], or a label inside the length that is outside
 *                  [0, alphabet_size) or equals blank_label (such a label is never used as an index).  Length 0 is the all-blank path.
 *   best         : int32 [minibatch] arg-min of the costs (lowest index on ties; -1 when every cost is +inf); best_cost: f32 [minibatch], that
 *                  cost; log_norm: f32 [minibatch] = log sum_k exp(-costs[n][k]) (-inf when none is finite), so candidate k's posterior within
 *                  the lexicon is exp(-costs[n][k] - log_norm[n]).  The three may be NULL together: the third launch is skipped.
 * OCR_STATUS_INVALID, with nothing launched, for a NULL required operand, best / best_cost / log_norm partly NULL, a blank outside
 * [0, alphabet_size), a sample_stride other than 0 or num_candidates, a short workspace, minibatch > 65535, or a shape
 * ocr_ctc_score_supported refuses. */
int ocr_ctc_score_supported(int alphabet_size, int max_time, int max_label_len, int num_candidates);
int ocr_ctc_score_workspace_size(int alphabet_size, int max_time, int minibatch, size_t* bytes);
int ocr_ctc_score(const float* activations, const int* input_lengths, const int* cand_labels, const int* cand_lengths, int sample_stride,
                  int alphabet_size, int minibatch, int max_time, int num_candidates, int max_label_len, int blank_label,
                  float* costs, int* best, float* best_cost, float* log_norm, void* workspace, size_t workspace_bytes, void* stream);
/* Shallow fusion of scored candidates: costs[n][k] -= lm_score[n][k] in place (both f32 [minibatch, num_candidates], contiguous; lm_score is
 * what a language model or constraint adds to the candidate's log-probability, as ocr_ctc_beam_decode_lm returns it; +inf - (-inf) is +inf,
 * so "no string" stays "no string"), then best / best_cost / log_norm of the fused costs exactly as ocr_ctc_score computes them - with
 * lm_score all zero the costs keep their bits and the three outputs are ocr_ctc_score's.  1 <= minibatch <= 65535,
 * 1 <= num_candidates <= 65536, no operand NULL; anything else is OCR_STATUS_INVALID and nothing is launched. */
int ocr_ctc_score_fuse(float* costs, const float* lm_score, int minibatch, int num_candidates, int* best, float* best_cost, float* log_norm,
                       void* stream);
/* lexicon scoring on a prefix tree: the costs, best, best_cost and log_norm of ocr_ctc_score for ONE lexicon shared by every sample, of up to
 * 1048576 words (ocr_ctc_trie_supported: 1 <= alphabet_size <= 16384, max_time >= 1, 1 <= num_words <= 1048576; arithmetic only).  Every node
 * of the lexicon's prefix tree runs the alpha recursion of its label slot and of the blank slot behind it once, whatever the number of words
 * below it, so the work is max_time x nodes instead of max_time x sum(2 L + 1).
 * ocr_ctc_trie_build (host code, no GPU) turns a dense lexicon (words int32 [num_words][max_label_len], lengths int32 [num_words], the layout
 * of ocr_ctc_score) into a CHUNKED tree: the words are sorted lexicographically and the sorted order is cut into contiguous ranges whose own
 * tries have at most chunk_nodes nodes each, the root and the ancestors shared with a neighbouring range included (a chunk is one workgroup's
 * work; ocr_ctc_trie_chunk_capacity() = 8192 is the most a workgroup holds).  Two passes: with nodes == NULL it writes only *num_chunks and
 * *num_nodes; with the five arrays given, and *num_chunks / *num_nodes holding what the arrays were sized for, it fills
 *   nodes            : int32 [*num_nodes], chunk after chunk.  A record = label | parent << 14 | flag << 27: parent is the index within the
 *                      chunk (parent < child; node 0 of a chunk is the root, label = blank_label, its own parent), flag = the node may take its
 *                      parent's non-blank mass (its label differs from the parent's);
 *   chunk_node_start : int32 [*num_chunks + 1], chunk_word_start: int32 [*num_chunks + 1]: prefix sums over nodes and over sorted words;
 *   word_node        : int32 [num_words], per word in sorted order its terminal node within its chunk; word_index: int32 [num_words], its index
 *                      in the caller's order.  Equal words share a node.  A word ocr_ctc_score would price +inf for every sample (a length
 *                      outside [0, max_label_len] or above 255, a label inside the length outside [0, alphabet_size) or equal to the blank) is
 *                      never inserted: node -1, in chunk 0.  Words at or beyond a word's length are never read.
 * OCR_ERR_INVALID for num_words < 1 or above 1048576, chunk_nodes below (longest valid word + 1) or above the capacity, a blank outside
 * [0, alphabet_size), NULL operands, or arrays too small.
 * ocr_ctc_score_trie: three launches on `stream` (log-sum-exp rows into `workspace`, ocr_ctc_trie_workspace_size bytes; one workgroup per
 * (chunk, sample); arg-min and normaliser), no host synchronisation.  The arrays are device copies of the builder's, chunk_nodes an upper bound
 * of every chunk's node count (the value the tree was built with).  costs f32 [minibatch][num_words] in the caller's word order, +inf as
 * ocr_ctc_score defines it; best / best_cost / log_norm as there, NULL together to skip the third launch.  OCR_ERR_INVALID, with nothing
 * launched, for a NULL operand, partly NULL outputs, a blank outside [0, alphabet_size), a short workspace, chunk_nodes outside
 * [1, capacity], num_chunks outside [1, num_words + 1], minibatch > 65535, or a shape ocr_ctc_trie_supported refuses. */
int ocr_ctc_trie_chunk_capacity(void);
int ocr_ctc_trie_supported(int alphabet_size, int max_time, int num_words);
int ocr_ctc_trie_build(const int* words, const int* lengths, int num_words, int max_label_len, int alphabet_size, int blank_label,
                       int chunk_nodes, int* num_chunks, int* num_nodes, int* nodes, int* chunk_node_start, int* chunk_word_start,
                       int* word_node, int* word_index);
int ocr_ctc_trie_workspace_size(int alphabet_size, int max_time, int minibatch, size_t* bytes);
int ocr_ctc_score_trie(const float* activations, const int* input_lengths, const int* nodes, const int* chunk_node_start,
                       const int* chunk_word_start, const int* word_node, const int* word_index, int num_chunks, int chunk_nodes,
                       int alphabet_size, int minibatch, int max_time, int num_words, int blank_label, float* costs, int* best,
                       float* best_cost, float* log_norm, void* workspace, size_t workspace_bytes, void* stream);
/* ctc_topk.hip.  The k best of a lexicon: for every row n of costs (f32, N rows of K entries, row stride ld >= K floats, any 4-byte aligned
 * base: a row-strided view of a larger matrix is fine) the k entries that are smallest under the total order "cost as a float, -0.0 == +0.0,
 * then the lower index", ascending.  +inf entries are never returned; NaN is outside the contract (the scorers produce none).
 * 1 <= k <= 64, 1 <= K <= 1048576 (ocr_ctc_topk_supported: arithmetic only), 1 <= N <= 65535.
 *   index    : int32 [N][k]; cost: f32 [N][k], the selected entries' own bits (signed zeros as stored); count: int32 [N] = min(k, finite entries
 *              of the row).  Slots at and beyond count[n] hold index -1, cost +inf, log_post -inf.
 *   log_post : f32 [N][k] = (-cost) - log_norm[n] (one fp32 negate and one subtract), or NULL.  log_norm: f32 [N] (what ocr_ctc_score writes), may
 *              be NULL; then log_post must be NULL too.
 * ocr_ctc_topk_plan (host only) reports how the launch cuts a row: `segments` pieces of `segment_len` entries (the last one shorter), a
 * workgroup per (segment, sample); one segment for rows of up to 8192 entries and wherever N alone fills the chip.  With more than one segment
 * a second launch merges the segments' k keys from `workspace` (ocr_ctc_topk_workspace_size bytes, 8-byte aligned; 0 bytes for a one-segment
 * plan, `workspace` may then be NULL).  The result is fully determined (no atomics, no dependence on workgroup order).  ocr_ctc_topk only
 * launches: no allocation, no synchronisation, no host read of device memory.  OCR_ERR_INVALID, with nothing launched, for a NULL costs /
 * index / cost / count, log_post without log_norm, ld < K, a short or missing workspace, or N, K, k out of range. */
int ocr_ctc_topk_supported(int K, int k);
int ocr_ctc_topk_plan(int N, int K, int k, int* segments, int* segment_len);
int ocr_ctc_topk_workspace_size(int N, int K, int k, size_t* bytes);
int ocr_ctc_topk(const float* costs, long ld, int N, int K, int k, const float* log_norm, int* index, float* cost, float* log_post,
                 int* count, void* workspace, size_t workspace_bytes, void* stream);
/* ctc_align.hip.  Forced alignment: the best (Viterbi) alignment of every candidate against the logits, with the operands, limits and the
 * meaning of "cannot be emitted" of ocr_ctc_score (num_candidates = 1 with sample_stride = 1 aligns each sample to its own transcript).
 *   start, end : int32 [minibatch][num_candidates][max_label_len], the first and last frame (inclusive, inside [0, input length)) the best
 *                path spends on character j; score: f32, same shape, the sum over those frames of act[t][n][label_j] - lse[t][n] added in
 *                ascending t; path_cost: f32 [minibatch][num_candidates], minus the log-probability of the best path.
 *   A candidate that cannot be emitted gets -1 / -1 / -inf in all max_label_len slots and path_cost +inf; one that can gets -1 / -1 / -inf in
 *   the slots at and beyond its length.  Length 0 is the all-blank path: no spans.
 * The recursion is max-plus in fp32 on ly = act - lse (no exp, no log): v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if the skip is
 * allowed) + ly; of equal values the smaller step wins (stay, then one slot, then two); the path ends in the last slot unless the one before
 * it is strictly better.  Two launches on `stream`: the log-sum-exp rows into the head of `workspace` (as ocr_ctc_score), then one wave per
 * (sample, candidate).  ocr_ctc_align_workspace_size: the lse table plus, when max_time > 64, 128 bytes per (sample, candidate, frame) of
 * back-pointers; OCR_ERR_INVALID above 2^40 bytes.  Every output word is written exactly once per call; no atomics.
 * OCR_ERR_INVALID, with nothing launched, for a NULL operand, a blank outside [0, alphabet_size), a sample_stride other than 0 or
 * num_candidates, a short workspace, minibatch > 65535, or a shape ocr_ctc_align_supported refuses (the ranges of ocr_ctc_score_supported). */
int ocr_ctc_align_supported(int alphabet_size, int max_time, int max_label_len, int num_candidates);
int ocr_ctc_align_workspace_size(int alphabet_size, int max_time, int minibatch, int num_candidates, int max_label_len, size_t* bytes);
int ocr_ctc_align(const float* activations, const int* input_lengths, const int* cand_labels, const int* cand_lengths, int sample_stride,
                  int alphabet_size, int minibatch, int max_time, int num_candidates, int max_label_len, int blank_label,
                  int* start, int* end, float* score, float* path_cost, void* workspace, size_t workspace_bytes, void* stream);
/* edit_distance.hip.  Levenshtein distance (unit costs for insert, delete and substitute) between every string of a set A and every string
 * of a set B, per sample: dist int32 [N][Ka][Kb].  String (n, i) of A starts at a + n * a_sn + i * a_ld (pitches and strides in ints) and has
 * the raw length a_len[n * Ka + i]; a_sn == 0 is one list shared by all samples, whose lengths are a_len[i].  B alike.  One entry so covers a
 * hypothesis against its truth (Ka = Kb = 1), the [N, K, T] paths of ocr_ctc_beam_decode_nbest against the truth or against themselves, and a
 * shared reference list.
 *   ignore  : a class whose occurrences are dropped from both strings before they are compared (the decoders' pad / ignore_value 0); -1 for
 *             none.  The counted length of a string is its raw length minus the dropped characters.
 *   "no string": a raw length below 0 (the empty slots of the n-best entry hold -1), a raw length above the pitch (a_ld / b_ld), or a counted
 *             length above 255.  Every pair with such a string gets dist = -1, and nothing else does.  No address at or beyond a string's
 *             start + pitch is read, whatever its length says.
 *   a_count, b_count: int32, indexed like a_len / b_len, the counted lengths, -1 for "no string"; either may be NULL.
 * 1 <= N <= 65535, 1 <= Ka, Kb <= 65536, N * Ka * Kb <= 2^30 (ocr_edit_distance_supported: arithmetic only).  One launch, a wave per four
 * consecutive pairs: where all their strings have at most 15 raw characters each pair gets 16 lanes, else the pairs take the whole wave in turn
 * (a column of the table per lane up to 63 counted characters of B, four per lane up to 255).  Integers only, fully determined: no atomics, no
 * communication between workgroups.  OCR_ERR_INVALID, with nothing launched, for a NULL a / a_len / b / b_len / dist, a negative pitch or
 * stride, a pointer that is not 4-byte aligned, or N, Ka, Kb out of range.
 * ocr_edit_stats: stats[4] (int64) = {sum of dist, sum of ref_count, number with dist == 0, number counted} over those of the M pairs (dist
 * and ref_count int32 [M]) with dist >= 0, in one launch of one workgroup: a validation batch leaves the device as four numbers.
 * 1 <= M <= 2^30; OCR_ERR_INVALID for a NULL operand, a stats that is not 8-byte aligned or M out of range.
 * ocr_mbr_select: minimum-Bayes-risk choice among the K candidates of every sample from their distances dist int32 [N][K][K] and costs f32
 * [N][K] (minus log-probabilities).  Candidate j is valid when costs[n][j] is finite and dist[n][j][j] >= 0; c_min = the least valid cost,
 * w_j = expf(c_min - c_j), Z = sum_j w_j, risk[n][i] = (sum_j w_j * dist[n][i][j]) / Z, both sums over the valid j in ascending order in
 * fp32 with one rounding per operation (the same bits whatever the launch); +inf for an invalid i.  best[n] = the arg-min under the total
 * order (risk, then cost, then the lower index), best_risk[n] its risk; -1 and +inf where no candidate is valid.  1 <= K <= 128, 1 <= N <= 65535;
 * OCR_ERR_INVALID, with nothing launched, for a NULL operand or N, K out of range. */
int ocr_edit_distance_supported(int Ka, int Kb, int N);
int ocr_edit_distance(const int* a, const int* a_len, long a_ld, long a_sn, int Ka, const int* b, const int* b_len, long b_ld, long b_sn,
                      int Kb, int N, int ignore, int* dist, int* a_count, int* b_count, void* stream);
int ocr_edit_stats(const int* dist, const int* ref_count, long M, long long* stats, void* stream);
int ocr_mbr_select(const int* dist, const float* costs, int N, int K, float* risk, int* best, float* best_risk, void* stream);
/* best-path decode (argmax, collapse repeats, drop blank): the greedy counterpart of
 * tf.nn.ctc_beam_search_decoder + sparse_tensor_to_dense(default 0) at network.py:656-657 / test.py:30-31.
 * decoded: int32 [minibatch, max_time] padded with pad_value; decoded_lengths: int32 [minibatch]. */
int ocr_ctc_greedy_decode(const float* activations, const int* input_lengths, int alphabet_size, int minibatch,
                          int max_time, int blank_label, int pad_value, int* decoded, int* decoded_lengths,
                          void* stream);

/* TF-semantics prefix beam search: tf.nn.ctc_beam_search_decoder(inputs, seq_len, beam_width=100, top_paths=1,
 * merge_repeated=True) as called at network.py:656 / test.py:30 — BLANK = alphabet_size-1, output dense + padded.
 * beam_width <= 128; neg_log_prob (may be NULL): f32 [minibatch].  Workspace from ocr_ctc_beam_workspace_size.
 * Coverage: 1 <= beam_width <= 128 and 2 <= alphabet_size <= 16384, by one of two kernels with the same semantics, outputs, workspace
 * layout and tie rule.  The table kernel keeps a score and a 16-bit child slot per (beam entry, class) in LDS and runs wherever
 *   4*roundup4(C) + 4*(K + K*C) + 2*roundup2(K*C) + 6656 bytes (rounded up to 16) <= 160 KB   (C = alphabet_size, K = beam_width:
 * C <= 259 at K = 100, C <= 202 at K = 128, C <= 15716 at K = 1; the query below answers for any shape).  Every other
 * covered shape runs the wide kernel, which scores only the min(K + 1, C - 1) likeliest non-blank classes of each frame (exact: DESIGN
 * section 6b) and needs 4*C + 4*K*(min(K + 1, C - 1) + 1) bytes plus the beam arrays.  Anything else is OCR_STATUS_INVALID from both
 * entry points, and nothing is launched. */
int ocr_ctc_beam_workspace_size(int alphabet_size, int minibatch, int max_time, int beam_width, size_t* bytes);
int ocr_ctc_beam_decode(const float* activations, const int* input_lengths, int alphabet_size, int minibatch,
                        int max_time, int beam_width, int merge_repeated, int pad_value, int* decoded,
                        int* decoded_lengths, float* neg_log_prob, void* workspace, size_t workspace_bytes, void* stream);
/* The same search with TF's top_paths and any blank class: the top_paths best prefixes of the final beam per sample, best first under the
 * total order (log-probability descending, then the lower beam slot); entries of probability zero are never returned.
 *   decoded: int32 [minibatch, top_paths, max_time] padded with pad_value; decoded_lengths: int32 [minibatch, top_paths];
 *   neg_log_prob: f32 [minibatch, top_paths]; count: int32 [minibatch], the number of paths returned (the beam may hold fewer than
 *   top_paths prefixes: C - 1 < top_paths, or few frames).  Slots at and beyond count[n] hold pad_value / length -1 / +inf: -1 is what
 *   ocr_ctc_score and ocr_ctc_align read as "no string", 0 is the empty string.
 * 1 <= top_paths <= beam_width <= 128 and 0 <= blank < alphabet_size; none of the operands may be NULL.  Workspace, kernel choice and
 * ocr_set_beam_engine as for ocr_ctc_beam_decode; anything else is OCR_STATUS_INVALID and nothing is launched.
 * blank = 0 with merge_repeated = 0 is the textbook CTC prefix search: its prefixes are label strings and neg_log_prob is comparable
 * with ocr_ctc_score(blank_label = 0), which it never undercuts (the beam sums a subset of the string's alignments).
 * blank = alphabet_size - 1, top_paths = 1 returns ocr_ctc_beam_decode's outputs bit for bit. */
int ocr_ctc_beam_decode_nbest(const float* activations, const int* input_lengths, int alphabet_size, int minibatch,
                              int max_time, int beam_width, int top_paths, int blank, int merge_repeated, int pad_value,
                              int* decoded, int* decoded_lengths, float* neg_log_prob, int* count, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The prefix search of ocr_ctc_beam_decode_nbest (any blank, no merge_repeated) fused with a deterministic weighted automaton over the
 * labels - a language model or a constraint inside the search, not after it.  The automaton has num_states states, start state 0 and
 *   lm_next: int32 [num_states, alphabet_size], lm_weight: f32 [num_states, alphabet_size], lm_final: f32 [num_states],
 * row-major and indexed by the caller's class ids; the blank's column is ignored.  Extending a prefix in state s by class c pays
 * lm_weight[s][c] and moves to lm_next[s][c]; the transition is forbidden (never a candidate, never a node) when the weight is not
 * finite (-inf, +inf, NaN) or lm_next[s][c] lies outside [0, num_states) - every entry is bounds-checked, no table content makes the
 * kernel read outside the tables.  The search keeps, prunes and ranks by
 *   total(P) = log p_beam(P | activations) + W(P),   W(P) = sum of the weights along P,
 * and the final ranking adds lm_final[state(P)]: a prefix whose lm_final is not finite may not end there and is not returned.
 *   decoded, decoded_lengths, count: as ocr_ctc_beam_decode_nbest; neg_log_prob: f32 [minibatch, top_paths] = -(total + lm_final);
 *   lm_score: f32 [minibatch, top_paths] = W(P) + lm_final, so -neg_log_prob - lm_score is the beam's acoustic log-probability of the
 *   string (comparable with ocr_ctc_score).  Slots at and beyond count[n] (which may be 0: the automaton can refuse everything) hold
 *   pad_value / -1 / +inf, and lm_score -inf.
 * Supported (ocr_ctc_beam_lm_supported, host-only, 1 / 0): 1 <= beam_width <= 128, 1 <= num_states <= 1048576, and the table kernel's LDS
 * (see ocr_ctc_beam_decode) plus 2048 bytes <= 160 KB: alphabet_size <= 256 at beam_width 100, <= 200 at 128.  The workspace
 * (ocr_ctc_beam_lm_workspace_size) is larger than ocr_ctc_beam_workspace_size's: each node also holds its state and its weight.
 * 1 <= top_paths <= beam_width, 0 <= blank < alphabet_size, none of the operands may be NULL; anything else is OCR_STATUS_INVALID,
 * nothing is launched and no output is written.  With one state, weights 0 and final 0 the outputs are ocr_ctc_beam_decode_nbest's
 * (merge_repeated = 0) bit for bit and lm_score is 0. */
int ocr_ctc_beam_lm_supported(int alphabet_size, int beam_width, int num_states);
int ocr_ctc_beam_lm_workspace_size(int alphabet_size, int minibatch, int max_time, int beam_width, size_t* bytes);
int ocr_ctc_beam_decode_lm(const float* activations, const int* input_lengths, int alphabet_size, int minibatch, int max_time,
                           int beam_width, int top_paths, int blank, int pad_value,
                           const int* lm_next, const float* lm_weight, const float* lm_final, int num_states,
                           int* decoded, int* decoded_lengths, float* neg_log_prob, float* lm_score, int* count,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The fused search for wide alphabets: ocr_ctc_beam_decode_lm with the automaton in a sparse form with failure (back-off) transitions, whose
 * size follows the arcs that exist (automaton.SparseLabelAutomaton).  num_states = H states, start state 0, num_arcs = A arcs:
 *   arc_begin: int32 [H + 1], the arcs of state s are arc_begin[s] .. arc_begin[s + 1] - 1;  arc_label: int32 [A], the caller's class ids,
 *   ascending within a state;  arc_next: int32 [A];  arc_weight: f32 [A];  backoff: int32 [H] (-1 = none);  backoff_weight: f32 [H];
 *   lm_final: f32 [H].
 * Reading class c in state s: the arcs of s are searched for c by bisection.  A hit pays the accumulated back-off weights plus arc_weight
 * (summed in float32 in hop order, the arc weight last) and moves to arc_next; it is forbidden when arc_weight or the sum is not finite or
 * arc_next lies outside [0, H).  A miss pays backoff_weight[s] and retries in backoff[s] when that lies in [0, H) and the weight is finite,
 * at most 8 times; otherwise the transition is forbidden.  Every arc range is clamped to [0, A] (an inverted one is empty) and every
 * arc_next and backoff is bounds-checked: no array content makes the kernel read outside the arrays or loop; labels that are not
 * ascending only make lookups miss.
 * New children of a frame are restricted to its min(cutoff, alphabet_size - 1) likeliest non-blank classes (ties at the boundary to the
 * lowest class), 1 <= cutoff <= beam_width + 1: with weights in the search this acoustic pruning is part of the result, not an exact
 * shortcut.  A child that is already in the beam receives its parent's mass whatever its class.  Everything else - total, ranking,
 * outputs, the slots beyond count[n], the workspace layout and size - is ocr_ctc_beam_decode_lm's.
 * Supported (ocr_ctc_beam_lm_sparse_supported, host-only, 1 / 0): 2 <= alphabet_size <= 16384, 1 <= beam_width <= 128, the cutoff range
 * above, 1 <= num_states <= 1 << 24, 0 <= num_arcs <= 1 << 28, and the wide kernel's LDS at min(cutoff, alphabet_size - 1) candidate classes
 * plus 2048 bytes <= 160 KB (which holds for every such shape).  It always runs the wide kernel, whatever ocr_set_beam_engine says.
 * 1 <= top_paths <= beam_width, 0 <= blank < alphabet_size, none of the operands may be NULL; anything else is OCR_STATUS_INVALID,
 * nothing is launched and no output is written.  With one state, an arc of weight 0 to itself for every class, final 0 and
 * cutoff = beam_width + 1 the outputs are the wide kernel's ocr_ctc_beam_decode_nbest (merge_repeated = 0) bit for bit, lm_score 0. */
int ocr_ctc_beam_lm_sparse_supported(int alphabet_size, int beam_width, int cutoff, int num_states, int num_arcs);
int ocr_ctc_beam_lm_sparse_workspace_size(int alphabet_size, int minibatch, int max_time, int beam_width, size_t* bytes);
int ocr_ctc_beam_decode_lm_sparse(const float* activations, const int* input_lengths, int alphabet_size, int minibatch, int max_time,
                                  int beam_width, int cutoff, int top_paths, int blank, int pad_value,
                                  const int* arc_begin, const int* arc_label, const int* arc_next, const float* arc_weight,
                                  const int* backoff, const float* backoff_weight, const float* lm_final, int num_states, int num_arcs,
                                  int* decoded, int* decoded_lengths, float* neg_log_prob, float* lm_score, int* count,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* Which kernel ocr_ctc_beam_decode runs for a shape - a host-only query like ocr_conv3x3_kernel_choice (nothing is launched, works
 * without a GPU): 0 refused, 1 table kernel, 2 wide kernel.  It honours ocr_set_beam_engine. */
int ocr_ctc_beam_kernel_choice(int alphabet_size, int beam_width);
/* A/B + test knob: 0 (default) = the table kernel wherever it fits, the wide kernel elsewhere; 2 = the wide kernel for every shape it
 * covers (alphabet_size <= 16384).  OCR_STATUS_INVALID for any other value. */
int ocr_set_beam_engine(int engine);

/* ---- dense contractions (tf.nn.conv2d network.py:166, tf.matmul :126, LSTMCell matmul :104-107) ------------- */
/* out[m][n] = sum_k P[m][k] * Q[n][k] (+bias[n]) ; bf16 operands, fp32 accumulate, K % 8 == 0, N % 4 == 0.
 * physical P row = m + (m / row_group) * row_skip when row_group > 0 (conv5's overlapping 2x2 VALID windows). */
int ocr_gemm_nt_bf16(const void* P, long ldp, const void* Q, long ldq, void* out, long ldo, int M, int N, int K,
                     const float* bias, const void* mask, long ldmask, int flags, int splits, int row_group,
                     int row_skip, int swap_inner, int swap_outer, void* stream);
/* engine selector for A/B measurements: 1 (default) = tap-reuse convolution kernels (conv_ws / conv_k3 / conv_k2 / conv_halo, chosen per
 * shape: DESIGN section 3) + 256-row LDS-DMA GEMM tiles, 0 = 128x128 register-staged tiles, 2 / 3 = LDS-DMA tiles without the tap-reuse
 * kernels; OCR_STATUS_INVALID for any other value */
int ocr_set_gemm_engine(int use_large_tile);
/* 3x3 SAME stride-1 convolution, x bf16 [Nb,W,H,Cin], wpack bf16 [Cout][3][3][Cin], y [Nb,W,H,Cout]
 * (conv_single network.py:160-191; also its data gradient with flipped/transposed weights).  The result does not depend on which kernel
 * the dispatcher takes beyond fp32 summation order (ocr_set_gemm_engine and the environment knobs OCR_CONV_K2 / OCR_CONV_K3 / OCR_K2_CFG /
 * OCR_CONV_WS select among them for the parity tests: the whole list, and the test file that forces each, is DESIGN section 8). */
int ocr_conv3x3_bf16(const void* x, const void* wpack, void* y, int Nb, int W, int H, int Cin, int Cout,
                     const float* bias, const void* mask, int flags, void* stream);
/* The convolution that also leaves the batch-norm statistics of its output behind (network.py:173-178: conv -> bias -> batch_norm):
 * partials = float [rows][2][Cout] with rows = ocr_conv3x3_stats_rows(...) = Nb*W*H / 256: per 256-pixel tile the per-channel sum and sum
 * of squares of the bf16 values that were stored (what a statistics pass over y would read).  Only where the plane-layout kernels take the
 * shape: the query returns 0 otherwise and the call OCR_STATUS_INVALID (run ocr_conv3x3_bf16 + ocr_bn_train_fwd then).  flags: BIAS / RELU. */
int ocr_conv3x3_stats_rows(int Nb, int W, int H, int Cin, int Cout, int flags);
int ocr_conv3x3_bf16_stats(const void* x, const void* wpack, void* y, int Nb, int W, int H, int Cin, int Cout, const float* bias, int flags,
                           float* partials, void* stream);
/* Which kernel family the two convolution entry points run for a shape — a host-only query (nothing is launched, works without a GPU):
 * 0 generic GEMM engines, 1 conv_halo, 2 / 3 conv_k2 tile A (256 x 128) / D (256 x 64), 4 / 5 conv_k3 A / D, 6 / 7 conv_k3w (tiles that
 * cross image boundaries) A / D, 8 conv_ws (weights in registers, persistent over the pixel tiles: Cin = 64 / 128 at H = 16 / 8); a NEGATIVE value (-OCR_STATUS_INVALID) for non-positive sizes.  flags as for ocr_conv3x3_bf16;
 * (kw, kh) = (0, 0) or the window of the fused max-pool. */
int ocr_conv3x3_kernel_choice(int Nb, int W, int H, int Cin, int Cout, int flags, int kw, int kh);
/* non-zero: ocr_conv3x3_bf16 accepts OCR_EPI_ACCUM for this shape (y (bf16) += result: the data gradient of a tensor with several
 * consumers is added to what was already delivered, no scratch tensor + add pass) */
int ocr_conv3x3_accum_supported(int Nb, int W, int H, int Cin, int Cout);
/* diagnostic: workgroup 0 of the convolution kernels (conv_halo, conv_k3 / conv_k3w) stamps {shader clock counter, 100 MHz wall clock} at entry ([0], [1]) and exit ([2], [3])
 * into dbg (device int64[8]; NULL = off) and adds its lifetime to [4] (shader clocks), [5] (wall ticks), [6] (launches) */
int ocr_conv_halo_clock_debug(void* dbg);
/* diagnostic: every workgroup of the weight-stationary convolution kernel (conv_ws) stamps the 100 MHz wall clock per phase and tile into
 * dbg (device int64[workgroups * 64]; NULL = off) — tools/ws_phases.py */
int ocr_conv_ws_debug(void* dbg);
/* conv3x3 + bias + ReLU AND the max-pool behind it from one epilogue (LSTM_train.py:26-33): y [Nb,W,H,Cout] and pooled
 * [Nb, W/kw, H/kh, Cout]; (kw, kh) = (1, 2) (feature axis) or (2, 2).  ocr_conv3x3_pool_supported() != 0 tells whether the shape is
 * covered; otherwise run ocr_conv3x3_bf16 + ocr_maxpool_fwd (ocr_conv3x3_relu_pool_bf16 then returns 2). */
int ocr_conv3x3_pool_supported(int Nb, int W, int H, int Cin, int Cout, int kw, int kh);
/* The training form: the same launch also writes the pool's routing codes (uint32 [Nb * W/kw * H/kh][Cout / 8], the format of
 * ocr_maxpool_bwd_codes) and, when y is NULL, no full-resolution tensor.  Only where ocr_conv3x3_pool_codes_supported() != 0 (the kernel planned
 * for the shape is conv_ws or an aligned-width conv_k3); elsewhere keep y and use ocr_conv3x3_relu_pool_bf16 + ocr_maxpool_bwd. */
int ocr_conv3x3_pool_codes_supported(int Nb, int W, int H, int Cin, int Cout, int kw, int kh);
int ocr_conv3x3_relu_pool_codes_bf16(const void* x, const void* wpack, void* y, void* pooled, void* codes, int Nb, int W, int H, int Cin,
                                     int Cout, const float* bias, int kw, int kh, void* stream);
int ocr_conv3x3_relu_pool_bf16(const void* x, const void* wpack, void* y, void* pooled, int Nb, int W, int H, int Cin, int Cout,
                               const float* bias, int kw, int kh, void* stream);
/* The data gradient of a convolution whose producer is such a pool, with the pool's backward pass in its write-out: conv3x3(dy, wdgrad) is
 * computed at the pooled resolution [Nb, W, H] and ONLY the full-resolution gradient out_full [Nb, W*kw, H*kh, Cout] is stored, routed by the
 * codes (uint32 [Nb*W*H][Cout / 8]) as ocr_maxpool_bwd_codes routes it (relu_mask: the winner's ReLU bit too) — bit-identical to
 * ocr_conv3x3_bf16 on an aligned-width conv_k3 kernel + ocr_maxpool_bwd_codes, every byte of out_full written.  Only where
 * ocr_conv3x3_unpool_supported() != 0 (the aligned-width conv_k3 instances: H in {4, 8}, W % (256 / H) == 0, Nb*W*H % 256 == 0,
 * Cin % 64 == 0, Cout % 64 == 0); otherwise the call returns 2 and launches nothing. */
int ocr_conv3x3_unpool_supported(int Nb, int W, int H, int Cin, int Cout, int kw, int kh);
int ocr_conv3x3_dgrad_unpool_bf16(const void* dy, const void* wdgrad, void* out_full, const void* codes, int Nb, int W, int H, int Cin,
                                  int Cout, int kw, int kh, int relu_mask, void* stream);
/* out[I][ldo] (f32) += scale * A^T B, A bf16 [Mk][lda], B bf16 [Mk][ldb]  (weight gradients of matmul layers);
 * colsum (may be NULL): colsum[j] += scale * sum_m B[m][j] — the bias gradient, produced by the same pass */
int ocr_gemm_tn_bf16(const void* A, long lda, const void* B, long ldb, float* out, long ldo, int Mk, int I, int J,
                     int row_group, int row_skip, long a_row_off, float scale, int splits, float* colsum, void* stream);
/* The same product (plain rows: no row group, no offset) without float atomics: every split of the contraction stores its partial block
 * to `part` and a second launch adds the splits in a fixed order, so out / colsum get the same bits in every run.  part holds at least
 * ocr_gemm_tn_split_workspace_floats(Mk, I, J) floats (-1: invalid shape). */
long ocr_gemm_tn_split_workspace_floats(int Mk, int I, int J);
int ocr_gemm_tn_split_bf16(const void* A, long lda, const void* B, long ldb, float* out, long ldo, int Mk, int I, int J, float scale,
                           float* colsum, float* part, long part_floats, void* stream);
/* nbatch products of one shape in one launch; problem b: A + b*strideA, B + b*strideB, out + b*strideOut, colsum + b*strideColsum */
int ocr_gemm_tn_batched_bf16(const void* A, long lda, long strideA, const void* B, long ldb, long strideB, float* out, long ldo,
                             long strideOut, int Mk, int I, int J, int nbatch, float scale, int splits, float* colsum,
                             long strideColsum, void* stream);
/* Round 4: several plain weight-gradient products in ONE launch of the ping-pong kernel (csrc/gemm_tn3.hip): one workgroup per 128 x 128
 * output tile over the whole contraction - no split over m, no atomics, bit-reproducible.  For every job and b < nbatch:
 *     out_b[I][J] += scale * A_b^T B_b,   colsum_b[J] += scale * column sums of B_b   (colsum may be NULL)
 * with A_b = A + b*strideA ([Mk rows][lda], rows in groups of row_group with row_skip unused rows behind each group; 0 = plain), B_b = B +
 * b*strideB, element strides.  jobs is a HOST array of 1 or 2 descriptors.  Needs I % 128 == 0, J % 128 == 0, Mk >= 256, 16-byte aligned
 * rows: ocr_gemm_tn_jobs_supported tells beforehand (host-only); OCR_STATUS_INVALID otherwise (use ocr_gemm_tn_bf16 / _batched_bf16). */
typedef struct ocr_tn_job {
    const void* A; long lda; long strideA;
    const void* B; long ldb; long strideB;
    float* out; long ldo; long strideOut;
    float* colsum; long strideColsum;
    int Mk, I, J, nbatch;
    int row_group, row_skip;
    float scale; int reserved;
} ocr_tn_job;
int ocr_gemm_tn_jobs_supported(const ocr_tn_job* jobs, int njobs);
int ocr_gemm_tn_jobs_bf16(const ocr_tn_job* jobs, int njobs, void* stream);
/* Two such jobs AND an independent plain GEMM (ocr_gemm_nt_bf16's arguments without `splits`) in ONE launch: the jobs' tiles hold one CU each
 * (128 KiB of LDS) and leave the other CUs idle; the GEMM's 256 x 128-tile workgroups run there.  Computes what ocr_gemm_tn_jobs_bf16(jobs, 2)
 * and ocr_gemm_nt_bf16(...) compute, bit for bit; neither part may read what the other writes.  ocr_gemm_tn_jobs_nt_supported (host-only,
 * nothing launched) is the policy: two covered jobs whose tiles leave at least a quarter of the CUs free, a GEMM with K % 64 == 0, N % 4 == 0,
 * N >= 128, M >= 1024 and no accumulate flag.  OCR_STATUS_INVALID otherwise: nothing was launched, issue the two launches. */
int ocr_gemm_tn_jobs_nt_supported(const ocr_tn_job* jobs, int njobs, int M, int N, int K, int flags);
int ocr_gemm_tn_jobs_nt_bf16(const ocr_tn_job* jobs, int njobs, const void* P, long ldp, const void* Q, long ldq, void* out, long ldo,
                             int M, int N, int K, const float* bias, const void* mask, long ldmask, int flags, int row_group,
                             int row_skip, int swap_inner, int swap_outer, void* stream);
/* A/B knob: 2 (default) = nine-tap slab kernel for conv weight gradients when a workspace is given (else as 1);
 * 1 = LDS-DMA per-tap tiles + fp32 atomics where I,J % 128 == 0; 0 = register-staged kernel */
int ocr_set_wgrad_engine(int engine);
/* dw f32 [3][3][Cin][Cout] (TF HWIO) += conv weight gradient; dbias (may be NULL) += sum over pixels of dy */
int ocr_conv3x3_wgrad_bf16(const void* x, const void* dy, float* dw, float* dbias, int Nb, int W, int H, int Cin,
                           int Cout, int splits, void* stream);
/* Which kernel computes that weight gradient - a host-only query like ocr_conv3x3_kernel_choice (nothing is launched, works without a
 * GPU; the dispatchers' own decisions, which the launches read too).  has_workspace != 0: as called through ocr_conv3x3_wgrad_ws_bf16 /
 * _defer_bf16 with a workspace of ocr_conv3x3_wgrad_workspace_size bytes; 0: ocr_conv3x3_wgrad_bf16.  Returns kernel | S << 8 with S the
 * number of splits of the pixel contraction (slabs of the slab kernels, atomic partial sums of the others) and kernel =
 * 0 wgrad9_kernel, 1 / 2 wgrad9p<4> / <8> (plane layout, whole-image steps), 3 / 4 their zero-row instances (general widths),
 * 5 gemm_tn2 nine-tap, 6 gemm_tn2 paired-tap (Cin = 64), 7 / 8 gemm_tn_kernel<1, 4, 4> / <1, 2, 2> (register-staged 128 x 128 / 64 x 64
 * tiles); a NEGATIVE value (-OCR_STATUS_INVALID) for sizes the entry points refuse.  Depends on ocr_set_wgrad_engine and on the knobs
 * OCR_W9_PLANES / OCR_W9P_GENW. */
int ocr_conv3x3_wgrad_kernel_choice(int Nb, int W, int H, int Cin, int Cout, int has_workspace, int splits);

/* the same through a caller-owned workspace of ocr_conv3x3_wgrad_workspace_size() bytes (0: shape not covered, the call then
 * behaves like ocr_conv3x3_wgrad_bf16): all nine taps from one staged tile, per-split partial slabs summed in a fixed order by a
 * second kernel — no atomics, bit-reproducible.  The workspace is scratch: neither zeroed by the caller nor kept. */
int ocr_conv3x3_wgrad_workspace_size(int Nb, int W, int H, int Cin, int Cout, size_t* bytes);
int ocr_conv3x3_wgrad_ws_bf16(const void* x, const void* dy, float* dw, float* dbias, int Nb, int W, int H, int Cin,
                              int Cout, int splits, void* workspace, size_t workspace_bytes, void* stream);
/* Deferred form: a backward pass may keep the partial slabs of all its layers (one workspace per layer) and reduce them in ONE launch at
 * its end — the per-layer reduce kernels are short and each is a dependent-kernel boundary.  Where the slab kernel covers the shape only it
 * runs here: `job` (64 bytes of HOST memory) receives the pending reduction, *job_blocks its block count, *deferred = 1, and the
 * workspace must stay untouched until ocr_wgrad9_reduce_jobs has run; otherwise the whole weight gradient is computed at once
 * (*deferred = 0).  ocr_wgrad9_reduce_jobs takes a DEVICE table of such jobs whose int at byte offset 60 (`block_start`) the caller
 * has set to the running sum of the preceding jobs' block counts; results are bit-identical to the per-layer form. */
int ocr_conv3x3_wgrad_defer_bf16(const void* x, const void* dy, float* dw, float* dbias, int Nb, int W, int H, int Cin, int Cout,
                                 void* workspace, size_t workspace_bytes, void* job, int* job_blocks, int* deferred, void* stream);
int ocr_wgrad9_reduce_jobs(const void* jobs, int njobs, int total_blocks, void* stream);
/* Two layers' slab kernels in ONE launch, for a layer whose own grid leaves half the chip idle: the first layer's workgroups are dispatched
 * in front, the second layer's behind them in the same grid.  Each layer is planned exactly as ocr_conv3x3_wgrad_defer_bf16 plans it (same
 * split count, same slabs: every slab word equals the single launch's), and job0 / job1 receive the two pending reductions.  shape =
 * {Nb, W, H, Cin, Cout}.  ocr_conv3x3_wgrad_pair_supported (host-only, nothing launched) returns 1 when both shapes take a slab kernel, a
 * paired instance exists (first: wgrad9_kernel; second: any slab kernel) and the first grid is at most half the CU count; 0 otherwise;
 * -OCR_STATUS_INVALID for bad arguments.  The launch returns OCR_STATUS_INVALID for a pair that is not supported. */
int ocr_conv3x3_wgrad_pair_supported(const int* shape_first, const int* shape_second);
int ocr_conv3x3_wgrad_pair_defer_bf16(const void* x0, const void* dy0, float* dw0, float* dbias0, const int* shape0, void* workspace0,
                                      size_t workspace_bytes0, const void* x1, const void* dy1, float* dw1, float* dbias1, const int* shape1,
                                      void* workspace1, size_t workspace_bytes1, void* job0, void* job1, int* job_blocks0, int* job_blocks1,
                                      void* stream);

/* ---- conv1 (Cin = 1), pooling, batch-norm, reductions, packing (network.py:160-191, 343-350, 176-178) -------- */
int ocr_conv1_fwd(const float* x, const float* w, const float* bias, void* y, int Nb, int W, int H, int Cout,
                  int relu, void* stream);
int ocr_conv1_wgrad(const float* x, const void* dz, float* dw, float* db, int Nb, int W, int H, int Cout,
                    void* stream);
/* element-wise bf16 (n % 8 == 0): op 0 out = a + b (Network.add), 1 out = relu(a) (Network.relu), 2 out = b > 0 ? a : 0,
 * 3 out = relu(a + b) (add + relu of a residual block in one pass), 4 out += b > 0 ? a : 0 (ReLU backward accumulated) */
int ocr_eltwise_bf16(int op, const void* a, const void* b, void* out, long n, void* stream);
/* conv1 + ReLU + 2x2 max-pool in one pass (LSTM_train.py:24-25); the backward recomputes the window instead of reading a
 * stored 67 MB activation: p / dp are the POOLED map [Nb, W/2, H/2, Cout] */
int ocr_conv1_pool_fwd(const float* x, const float* w, const float* bias, void* p, int Nb, int W, int H, int Cout, void* stream);
/* training form.  codes (may be NULL; Cout == 64): uint32 [Nb * W/2 * H/2][8], 4 bits per pooled output = position of the window's first
 * maximum (bf16-rounded values, TF scan order) | ReLU bit << 2, consumed by ocr_conv1_pool_bwd_codes (bit-identical gradients without
 * recomputing the windows).  zero (may be NULL): fp32 [zero_n] cleared by the same launch (zero_n % 4 == 0, 16-byte aligned): the step's
 * flat gradient buffer.  ones (may be NULL): ones_n 32-bit words (% 4 == 0, 16-byte aligned) set to 0xFFFFFFFF by the same launch: the
 * hand-off blocks of the step's persistent LSTM launches (OCR_LSTM_PREPARED below). */
int ocr_conv1_pool_fwd_train(const float* x, const float* w, const float* bias, void* p, int Nb, int W, int H, int Cout,
                             void* codes, float* zero, long zero_n, void* ones, long ones_n, void* stream);
int ocr_conv1_pool_bwd_codes(const float* x, const float* w, const float* bias, const void* dp, float* dw, float* db,
                             int Nb, int W, int H, int Cout, const void* codes, void* stream);
/* slab form: no atomics - block b leaves {dW [9][64] | db [64]} (fp32) in slab[b][640], b < ocr_conv1_pool_bwd_slab_rows(Nb, W, H); the rows
 * are added by ocr_wgrad9_reduce_jobs (jobs with n4 = 144 / 16, slab4 = 160, S = rows): bit-reproducible.  codes may be NULL (recompute). */
int ocr_conv1_pool_bwd_slab_rows(int Nb, int W, int H);
int ocr_conv1_pool_bwd_slab(const float* x, const float* w, const float* bias, const void* dp, int Nb, int W, int H, int Cout,
                            const void* codes, float* slab, void* stream);
int ocr_conv1_pool_bwd(const float* x, const float* w, const float* bias, const void* dp, float* dw, float* db, int Nb,
                       int W, int H, int Cout, void* stream);
int ocr_maxpool_fwd(const void* x, void* y, int Nb, int W, int H, int C, int kw, int kh, void* stream);
int ocr_maxpool_bwd(const void* x, const void* dy, void* dx, int Nb, int W, int H, int C, int kw, int kh,
                    int relu_mask, void* stream);
/* ocr_maxpool_bwd from the pool's routing codes instead of its full-resolution input x: codes = uint32 [Nb * W/kw * H/kh][C / 8], one word per
 * (window, 8-channel group), 4 bits per channel - bits 0-1 the index of the window's first maximum in TF scan order (a * kh + b, a over W),
 * bit 2 maximum > 0 - as a forward pass that compares the bf16-rounded values writes them.  (kw, kh) = (2, 2) or (1, 2); dx is
 * bit-identical to ocr_maxpool_bwd's. */
int ocr_maxpool_bwd_codes(const void* codes, const void* dy, void* dx, int Nb, int W, int H, int C, int kw, int kh,
                          int relu_mask, void* stream);
/* training-mode batch norm over rows of x[M][C] (network.py:176-178): batch statistics, biased variance.  `workspace` is
 * ocr_bn_workspace_bytes(M, C) bytes of caller-owned scratch (per-block partial sums; neither zeroed nor kept) */
size_t ocr_bn_workspace_bytes(long M, int C);
/* residual (bf16 [M][C], may be NULL): y = [relu](bf16(bn(x)) + residual) — the tail of a residual block (bn, Network.add,
 * Network.relu) in the apply pass, bit-identical to the three separate passes */
int ocr_bn_train_fwd(const void* x, void* y, const float* gamma, const float* beta, float* save_mean,
                     float* save_rstd, long M, int C, float eps, int relu, void* workspace, const void* residual, void* stream);
int ocr_bn_train_bwd(const void* x, const void* y, const void* dy, void* dx, const float* gamma,
                     const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta, long M, int C,
                     int relu, void* workspace, void* stream);
/* Round 4 forms.  partial_rows > 0: the workspace already holds that many rows [rows][2][C] of per-tile sums / sums of squares written by
 * the producing convolution's epilogue (ocr_conv3x3_bf16_stats) - no statistics pass over x.  pooled (may be NULL): the 1 x 2 max-pool over
 * row pairs (2q, 2q + 1) that follows the layer (LSTM_train.py:33) is written by the apply pass too ([M / 2][C]; M even, no residual);
 * bit-identical to ocr_maxpool_fwd on y.  pooled_dy != 0: `dy` is the gradient of that pool ([M / 2][C]); both backward passes route it to
 * the first maximum of each row pair themselves - bit-identical to ocr_maxpool_bwd followed by ocr_bn_train_bwd. */
int ocr_bn_train_fwd2(const void* x, void* y, const float* gamma, const float* beta, float* save_mean, float* save_rstd, long M, int C,
                      float eps, int relu, void* workspace, const void* residual, int partial_rows, void* pooled, void* stream);
int ocr_bn_train_bwd2(const void* x, const void* y, const void* dy, void* dx, const float* gamma, const float* save_mean,
                      const float* save_rstd, float* dgamma, float* dbeta, long M, int C, int relu, void* workspace, int pooled_dy,
                      int partial_rows, void* stream);
/* The training forms where that pool is the layer's ONLY consumer: the apply pass writes pooled and the pool's routing codes (uint32 [M / 2][C / 8],
 * the format of ocr_maxpool_bwd_codes for the 1 x 2 window) and no y; the backward passes take the winner of each pair and its ReLU mask from
 * the codes.  dx, dgamma and dbeta are bit-identical to ocr_bn_train_bwd2(pooled_dy = 1) on the y of ocr_bn_train_fwd2. */
int ocr_bn_train_fwd_codes(const void* x, const float* gamma, const float* beta, float* save_mean, float* save_rstd, long M, int C,
                           float eps, int relu, void* workspace, int partial_rows, void* pooled, void* codes, void* stream);
int ocr_bn_train_bwd_codes(const void* x, const void* codes, const void* dy, void* dx, const float* gamma, const float* save_mean,
                           const float* save_rstd, float* dgamma, float* dbeta, long M, int C, int relu, void* workspace, void* stream);
/* ... with ocr_conv5_col2im inside the statistics pass: the pooled gradient [M / 2][C] = [Nb][W][HC] is formed from the column matrix `col` of
 * the full-height convolution behind the pool ([Nb * (W - 1)][2 * HC], M / 2 * C == Nb * W * HC) while the sums are taken, and stored to
 * dy_pooled_out for the apply pass.  dy_pooled_out, dx, dgamma and dbeta are bit-identical to ocr_conv5_col2im + ocr_bn_train_bwd_codes. */
int ocr_bn_train_bwd_codes_col(const void* x, const void* codes, const void* col, int Nb, int W, int HC, void* dy_pooled_out, void* dx,
                               const float* gamma, const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta, long M,
                               int C, int relu, void* workspace, void* stream);
/* partial_rows > 0 (not with pooled_dy): dy is ALREADY ReLU-masked and the workspace holds that many rows [rows][2][C] of (sum dz, sum dz *
 * xhat) from the data-gradient kernel that wrote dy — ocr_conv3x3_dgrad_bnbwd_bf16: dx = (mask_y > 0) ? conv3x3(dy, wdgrad) : 0 plus those
 * per-256-pixel-tile sums with xhat = (z - mean) * rstd, rows = ocr_conv3x3_bnbwd_rows(...) (0: shape not covered, use the separate passes).
 * The batch-norm backward of the producing layer then needs no statistics pass over (z, y, dy) and no second read of y. */
int ocr_conv3x3_bnbwd_rows(int Nb, int W, int H, int Cin, int Cout);
int ocr_conv3x3_dgrad_bnbwd_bf16(const void* dy, const void* wdgrad, void* dx, int Nb, int W, int H, int Cin, int Cout, const void* mask_y,
                                 const void* z, const float* mean, const float* rstd, float* partials, void* stream);
int ocr_colsum_bf16(const void* a, float* out, long M, int C, long lda, void* stream);
int ocr_pack_transpose(const float* in, void* out, int R, int Cc, long ldin, int lstm_units, void* stream);
int ocr_pack_conv_dgrad(const float* w, void* out, int Cin, int Cout, void* stream);
/* all weight re-packs of a step in ONE launch.  jobs: device array of 64-byte records
 * {int type(0 transpose+perm,1 conv-dgrad flip,2 strided cast,3 flat cast,4 LSTM bias [4*lstm_units] fp32 -> packed gate order, fp32 dst);
 *  int R, Cc, lstm_units; long ldin, ldout;
 *  const float* src; bf16* dst; long n; int block_start, nblocks;}  with block_start ascending */
int ocr_pack_jobs(const void* jobs, int njobs, int total_blocks, void* stream);
int ocr_cast_f32_bf16(const float* in, void* out, long n, void* stream);
/* uint8 pixels -> fp32 in [0, 1] (= u8 / 255, correctly rounded: identical to the host's `astype(float32) / 255.`, gen.py:59-65); n % 4 == 0 */
int ocr_u8_to_unit_f32(const void* in, float* out, long n, void* stream);
/* What train.py:130,139 fetches after sess.run, gathered on the device into out[4] (doubles): mean per-sample CTC cost, sum w^2 of
 * the regularised parameters (scalars[1]) and the global gradient norm (scalars[7]) of the optimiser block (scalars: NULL, or the WHOLE block of
 * ocr_optim_scalar_count() doubles — entry [72] is read too),
 * and a bit mask of the error words that read 1 — the persistent LSTM kernels' time-out mark; 0 and 0xFFFFFFFF (a caller-prepared block,
 * OCR_LSTM_PREPARED) both mean "nothing happened" (word_addrs: device array of nwords <= 32 device addresses of int error words); 2^40 is added
 * when the update of the step the report follows was dropped on the device (scalars[72], ocr_optim_step_guarded*). */
int ocr_step_report(const float* costs, int n, const double* scalars, const void* word_addrs, int nwords, double* out, void* stream);
/* One launch binding a DEVICE-resident batch to the engine's fixed input buffers (the feed_dict of train.py:126-130 once the
 * batch is already in HBM): pixels -> x (uint8 / 255 when pixels_are_u8, else an fp32 copy; n_pixels % 4 == 0) and the
 * int32 vectors seq_len, flat labels, labels_len (counts may be 0 for inference). */
int ocr_bind_batch(const void* pixels, int pixels_are_u8, float* x, long n_pixels, const int* seq_len, int* seq_len_dst, int n_seq,
                   const int* labels, int* labels_dst, int n_labels, const int* labels_len, int* labels_len_dst, int n_labels_len,
                   void* stream);
int ocr_cast2d_f32_bf16(const float* in, long ldin, void* out, long ldout, int rows, int cols, void* stream);
int ocr_tnc_to_ntc_bf16(const float* in, void* out, int T, int N, int C, float scale, void* stream);
int ocr_conv5_col2im(const void* col, void* dx, int Nb, int W, int HC, void* stream);

/* ---- layers of the reference DSL outside the shipped graphs (lstm_ctc_ocr_amd/csrc/dsl_ops.hip) --------------- */
/* stand-alone batch_normalization with the stored (moving) statistics — is_training=False, network.py:466-473 */
int ocr_bn_infer_fwd(const void* x, void* y, const float* gamma, const float* beta, const float* mean, const float* var,
                     long M, int C, float eps, int relu, void* stream);
int ocr_bn_infer_bwd(const void* x, const void* y, const void* dy, void* dx, const float* gamma, const float* mean,
                     const float* var, float* dgamma, float* dbeta, long M, int C, float eps, int relu, void* stream);
/* tf.nn.dropout (network.py:626-628): out = keep(i) ? in / keep_prob : 0; keep(i) = hash(seed, *step_counter, i) < keep_prob —
 * the same call with the same arguments on the gradient is the backward pass (nothing stored); step_counter: device double or NULL */
int ocr_dropout_bf16(const void* in, void* out, long n, unsigned seed, const void* step_counter, float keep_prob, void* stream);
/* tf.nn.avg_pool, window == stride in {1,2}^2 (network.py:352-359); backward: src = dy (pooled), dst = dx */
int ocr_avgpool_bf16(const void* src, void* dst, int Nb, int W, int H, int C, int kw, int kh, int backward, void* stream);
/* strided pick y[n,wo,ho,:] = x[n, wo*sw+ow, ho*sh+oh, :] (a strided convolution = stride-1 convolution + pick) / its transpose */
int ocr_subsample_bf16(const void* src, void* dst, int Nb, int W, int H, int C, int Wo, int Ho, int sw, int sh, int ow, int oh,
                       int backward, void* stream);
int ocr_softmax_f32(const float* in, float* out, long rows, int C, void* stream);     /* network.py:441-447, last axis */

/* ---- LSTM (bi_lstm network.py:97-129, lstm network.py:130-152; TF-1.0 LSTMCell gate order i,j,f,o, forget_bias 1.0) -----
 * ndir = 2: forward | backward direction (bidirectional_dynamic_rnn, backward reversed within each length);  ndir = 1: forward only
 * (dynamic_rnn).  Row strides of the per-step tensors follow it: xproj / dz [R][ndir][4U], hout / dhout [R][ndir*U],
 * gates [ndir][R][4U], cell [ndir][R][U]. */
int ocr_lstm_fwd_step(const float* xproj, const void* whT_packed, const int* seq_len, void* hout, float* gates,
                      float* cell, int Nb, int T, int U, int step, float forget_bias, int ndir, void* stream);
int ocr_lstm_bwd_step(const void* wh, long ldw, long w_dir_stride, const int* seq_len, const void* dhout,
                      const float* gates, const float* cell, void* dz, float* dc_state, int Nb, int T, int U,
                      int step, int ndir, void* stream);
/* whole-sequence (persistent) variants: one launch for all T steps.  The U/16 workgroups of a (direction, batch tile) group
 * exchange h_t / dz_t either through a small ring that stays in one XCD's L2 (protocol 4, default), through the output tensor
 * itself (protocol 2; the call first fills it with the bf16 pattern 0xFFFF = "not written yet") or behind counters (protocol 0) —
 * see ocr_set_lstm_proto.  `sync`: ocr_lstm_seq_sync_words(Nb, U) int32 words of scratch (group counters | ring | tail; what the
 * protocol needs is initialised by the call; LAST word = spin-timeout error flag, non-zero => results invalid).
 * ocr_lstm_seq_supported() tells whether the shape is covered (two directions, U == 256 or 512 — the latter with the contraction
 * axis split over two waves — and a grid of at most one workgroup per CU); otherwise use the step entry points. */
int ocr_lstm_seq_supported(int Nb, int U);
long ocr_lstm_seq_sync_words(int Nb, int U);
int ocr_lstm_seq_debug(void* dbg /* device int64[4*T] phase stamps of workgroup 0, NULL = off */);
/* test hook: in the persistent launches that follow, unit block 0 of EVERY (direction, batch tile) group sleeps units x 64 shader clocks at the
 * top of iteration `at` (at < 0: of every iteration; units 0 = off, the default; 0 .. 4096) — the skew between the workgroups of a group that HBM
 * contention produces once in ~10^4 launches, made deterministic: the ring hand-off that stands in for the dependent op sequence of
 * network.py:104-109 must be right for any relative speed of its workgroups (tests/test_gpu_stress.py, tools/lstm_ring_model.py).  Baked into a
 * captured graph at capture time. */
int ocr_lstm_seq_test_skew(int units, int at);
int ocr_lstm_fwd_seq(const float* xproj, const void* whT_packed, const int* seq_len, void* hout, float* gates,
                     float* cell, int Nb, int T, int U, float forget_bias, void* sync, void* stream);
int ocr_lstm_bwd_seq(const void* wh, long ldw, long w_dir_stride, const int* seq_len, const void* dhout,
                     const float* gates, const float* cell, void* dz, int Nb, int T, int U, void* sync, void* stream);
/* The same launches with flags.  OCR_LSTM_PREPARED: the caller has set EVERY word of `sync` to 0xFFFFFFFF earlier on this stream (the
 * training engine does that for all of a step's launches inside a kernel it runs anyway, ocr_conv1_pool_fwd_train) and the call's own
 * fill launch is skipped — under the ring protocol (4) only; under the counter protocol the call prepares the block itself as before.
 * The error word (last word of `sync`) of a caller-prepared block reads 0xFFFFFFFF when nothing happened and 1 after a time-out. */
#define OCR_LSTM_PREPARED 1
int ocr_lstm_fwd_seq2(const float* xproj, const void* whT_packed, const int* seq_len, void* hout, float* gates,
                      float* cell, int Nb, int T, int U, float forget_bias, void* sync, int flags, void* stream);
int ocr_lstm_bwd_seq2(const void* wh, long ldw, long w_dir_stride, const int* seq_len, const void* dhout,
                      const float* gates, const float* cell, void* dz, int Nb, int T, int U, void* sync, int flags, void* stream);
/* The forward recurrence WITH the input projection inside (no projection GEMM, no fp32 projection tensor): x bf16 [Nb * T][D] (the layer's
 * input rows, batch-major), wxT_packed bf16 [2][4U][D] and bias_packed fp32 [2][4U] exactly as the projection GEMM takes them
 * (ocr_pack_transpose with lstm_units, ocr_lstm_pack_bias).  Covered: ring protocol, 16-row tiles, four-wave workgroups, D = 512 / 1024,
 * U = 256 / 512 — ocr_lstm_fwd_seq_x_supported; otherwise OCR_ERR_INVALID (run the GEMM + ocr_lstm_fwd_seq2).  flags as above. */
int ocr_lstm_fwd_seq_x_supported(int Nb, int U, int D);
int ocr_lstm_fwd_seq_x(const void* x, const void* wxT_packed, const float* bias_packed, int D, const void* whT_packed,
                       const int* seq_len, void* hout, float* gates, float* cell, int Nb, int T, int U, float forget_bias,
                       void* sync, int flags, void* stream);
/* hand-off protocol of the persistent kernels: 4 (default) = data-as-flag through a ring inside one XCD's L2, 2 = data-as-flag
 * through the output tensor inside one XCD's L2 — both need workgroups with equal (id & 7) on one XCD, see ocr_probe_xcc;
 * 0 = counters (sc1): placement independent */
int ocr_set_lstm_proto(int proto);
/* waves per workgroup of the persistent kernels' 16-row tiles under protocol 4: 4 (default: the contraction axis, the polls and the gate
 * math of a step split over four waves) or 1 (the one-wave kernels of rounds 2-3).  Same tensors, same hand-off ring; results equal up to
 * fp32 summation order.  OCR_ERR_INVALID for other values.  The environment variable OCR_LSTM_KSPLIT (1 / 4) wins over this setter. */
int ocr_set_lstm_ksplit(int waves);
int ocr_lstm_hprev(const void* hout, const int* seq_len, void* hprev, int Nb, int T, int U, int ndir, void* stream);
/* xh [ndir][Nb*T][D+U] = [x | h_{t-1} in direction order]: operand of the LSTMCell-matrix weight gradient (one GEMM per direction) */
int ocr_lstm_xh(const void* x, const void* hout, const int* seq_len, void* xh, int Nb, int T, int D, int U, int ndir, void* stream);
int ocr_lstm_pack_bias(const float* b_fw, const float* b_bw /* NULL when ndir == 1 */, float* out, int U, int ndir, void* stream);

/* ---- optimiser (train.py:73-85: clip_by_global_norm 10.0 + Adam / Momentum / RMSProp; L2 of network.py:630-637) */
int ocr_optim_scalar_count(void);   /* doubles in the caller-owned `scalars` block: 8 of state + per-step partial-sum bins + 2 of the guard */
int ocr_optim_init(void* scalars /* ocr_optim_scalar_count() doubles */, double lr, void* stream);
int ocr_optim_set_lr(void* scalars, double lr, int multiply, void* stream);
int ocr_optim_step(float* params, float* grads, float* state1, float* state2, long n, long reg_begin, long reg_end,
                   float weight_decay, float clip_norm, int solver, float beta1, float beta2, float eps,
                   void* scalars, void* stream);
/* the same step behind a guard: guard_addrs = device array of nguard (<= 64) device addresses of int words that read 1 when a kernel of this step
 * reported invalid results (the persistent LSTM launches' error words: a bounded inter-workgroup wait expired).  The update is then dropped on the
 * device — moments, parameters and the bias-correction powers stay; scalars[72] = 1 for that step, scalars[73] counts the dropped steps. */
int ocr_optim_step_guarded(float* params, float* grads, float* state1, float* state2, long n, long reg_begin, long reg_end,
                           float weight_decay, float clip_norm, int solver, float beta1, float beta2, float eps,
                           void* scalars, const void* guard_addrs, int nguard, void* stream);
/* ... and / or behind a drop flag (data parallel, train.py:79-83 applied by every replica or by none): drop_flag = a device float, > 0 => drop
 * (NULL: none).  ocr_guard_flag writes 1.0f / 0.0f (any of the nguard words reads 1 / none does) into flag_out; a rank puts that word at the end of
 * its late gradient bucket, the SUM all-reduce turns it into the number of ranks whose step timed out, and every rank drops the SAME step.
 * scalars[74] counts the expired waits the guard has seen (error words that read 1 + ranks that raised the flag). */
int ocr_optim_step_guarded2(float* params, float* grads, float* state1, float* state2, long n, long reg_begin, long reg_end,
                            float weight_decay, float clip_norm, int solver, float beta1, float beta2, float eps,
                            void* scalars, const void* guard_addrs, int nguard, const float* drop_flag, void* stream);
int ocr_guard_flag(const void* guard_addrs, int nguard, float* flag_out, void* stream);

/* ---- GPU-side captcha synthesis (the data side of the path: /root/reference/lib/lstm/utils/gen.py:31-37 generateImg — captcha.ImageCaptcha on 12
 * worker processes — and :41-67 groupBatch: resize to height 32, [W, 32] rows, right-padded with 0) ---------------------------------------------
 * One workgroup per image composes resident glyph masks in LDS with Pillow's own arithmetic (affine bilinear rotation, DIV255 paste, bicubic
 * resize, noise dots + arc, 3 x 3 SMOOTH, bilinear resize) and writes out[n_images][W][out_h] uint8 — what ocr_bind_batch takes as pixels.
 * params: int32 [n_images][words_per_image] records (lstm_ctc_ocr_amd/utils/synth.draw_params: every random draw + the integer geometry;
 * max_glyphs glyph slots per record); atlas: concatenated 8-bit glyph masks (records hold byte offsets into it); stamp: n_stamp (dx, dy) int32
 * pairs = the footprint of one noise dot; canvas_cap / width_cap >= every record's canvas_w / width (they size the LDS image:
 * 60 * (canvas_cap + width_cap) + 34816 bytes <= 160 KB, else OCR_ERR_INVALID).  The records live in device memory: that they respect the two
 * caps, the atlas' extent and max_glyphs is the caller's contract and is NOT checked by the launch (utils/synth.draw_params produces records and
 * caps together). */
int ocr_captcha_synth(const int* params, int n_images, int words_per_image, int max_glyphs, const void* atlas, const int* stamp, int n_stamp,
                      void* out, int W, int out_h, int canvas_cap, int width_cap, void* stream);

/* diagnostics (experiments library; the product library stores the pointer and never reads it): wall-clock phase stamps of every wgrad9p_kernel
 * workgroup, device int64 [workgroups][8] (NULL = off); tools/w9p_phases.py */
int ocr_wgrad9_debug(void* dbg);

/* ---- device probes used by the test-suite (not part of the hot path) ------------------------------------------ */
/* ds_read_b64_tr_b16 lane-semantics probe: LDS holds shorts 0..8191 (value = element index); lane l reads at
 * byte offset addr[l]; out[l*4+j] = element j returned to lane l. */
int ocr_probe_tr16(const int* addr /* 64 */, int* out /* 64*4 */, void* stream);
/* out[id] = XCC_ID of workgroup id of a 1-D grid, out[nblocks + id] = its HW_ID register (evidence for id & 7 == XCD) */
int ocr_probe_xcc(int* out /* 2*nblocks */, int nblocks, int threads, void* stream);
/* one-GPU stand-in for the CUs a concurrent RCCL collective holds (torch.distributed all_reduce over xGMI: lib/lstm/train.py has no
 * counterpart — the reference is single-device): nblocks workgroups of `threads` threads with lds_bytes of LDS each stay
 * resident for `us` microseconds without issuing work.  Used by the OCR_FAKE_COMM_CUS / OCR_FAKE_COMM_US emulation (lstm_ctc_ocr_amd/dist.py). */
int ocr_occupy_cus(int nblocks, int threads, int lds_bytes, float us, void* stream);
/* counter calibration: every wave issues iters x 8 back-to-back v_mfma_f32_16x16x32_bf16 (a saturated matrix pipe with an exactly known
 * instruction count); clk[4] = {shader clock, 100 MHz clock} of workgroup 0 at loop entry and exit, or NULL (tools/mfma_busy_probe.py) */
int ocr_mfma_busy_probe(float* out, int nblocks, int threads /* multiple of 64, <= 512 */, int iters, long long* clk, void* stream);

#ifdef __cplusplus
}
#endif
#endif
