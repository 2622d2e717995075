"""Thin tensor-level wrappers over the C ABI (include/ocr_hip.h).

torch is used for allocation and stream handles only; every function enqueues hand-written HIP kernels on torch's
current stream and returns device tensors.  No function here has a CPU or eager fallback.
"""
import ctypes

import torch

from . import _native as nat
from ._native import EPI_ACCUM, EPI_BIAS, EPI_MASK, EPI_OUT_F32, EPI_RELU, EPI_ROWSWAP, call, ptr

BF16 = torch.bfloat16
F32 = torch.float32


def _st():
    return nat.stream()


def _dev(t):
    if not t.is_cuda:
        raise nat.NativeError("hot-path operators take device tensors only (got a CPU tensor)")
    return t


# ----------------------------------------------------------------------------------------------- CTC
def ctc_workspace_bytes(max_label_len, max_time, minibatch):
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_workspace_size", max_label_len, max_time, minibatch, ctypes.byref(sz))
    return sz.value


def ctc_loss(acts, flat_labels, label_lengths, input_lengths, max_label_len, blank=0, want_grad=True,
             workspace=None, costs=None, grads=None):
    """warp-ctc shaped: acts f32 [T, N, C] unnormalised; labels/lengths int32 device tensors."""
    T, N, C = acts.shape
    _dev(acts)
    if workspace is None:
        workspace = torch.empty(ctc_workspace_bytes(max_label_len, T, N), dtype=torch.uint8, device=acts.device)
    if costs is None:
        costs = torch.empty(N, dtype=F32, device=acts.device)
    if want_grad and grads is None:
        grads = torch.empty_like(acts)
    call("ocr_ctc_loss", ptr(acts), ptr(grads) if want_grad else None, ptr(flat_labels), ptr(label_lengths),
         ptr(input_lengths), C, N, T, max_label_len, blank, ptr(costs), ptr(workspace), _st())
    return costs, (grads if want_grad else None)


def ctc_train_supported(C, T, max_label_len):
    return bool(nat.lib().ocr_ctc_train_supported(C, T, max_label_len))


def ctc_loss_train(acts, grad_ntc_bf16, scale, flat_labels, label_lengths, input_lengths, max_label_len, costs, blank=0):
    """costs + scale * d cost / d acts written as bf16 [N, T, C] in one launch."""
    T, N, C = acts.shape
    call("ocr_ctc_loss_train", ptr(_dev(acts)), ptr(grad_ntc_bf16), float(scale), ptr(flat_labels), ptr(label_lengths),
         ptr(input_lengths), C, N, T, max_label_len, blank, ptr(costs), _st())
    return costs


def ctc_long_supported(C, T, max_label_len):
    return bool(nat.lib().ocr_ctc_long_supported(C, T, max_label_len))


def ctc_long_placement(C, T, max_label_len):
    """'lds' / 'workspace': where the long-label kernel keeps its [T][S] tables at this shape; None where it does not cover the shape."""
    return (None, 'lds', 'workspace')[nat.lib().ocr_ctc_long_placement(C, T, max_label_len)]


def ctc_long_workspace_bytes(C, max_label_len, max_time, minibatch):
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_long_workspace_size", C, max_label_len, max_time, minibatch, ctypes.byref(sz))
    return sz.value


def _ctc_loss_tables(entry, workspace_bytes, acts, labels, label_lengths, input_lengths, max_label_len, blank, want_grad, grad_ntc_bf16, scale,
                     workspace, costs, grads):
    """The long-label and wide-alphabet forms: one signature, `entry` the C entry point and `workspace_bytes` its size function (0 for the
    long form with its tables in LDS: one byte is allocated then; the wide form's is never 0)."""
    T, N, C = acts.shape
    _dev(acts)
    if workspace is None:
        workspace = torch.empty(max(workspace_bytes(C, max_label_len, T, N), 1), dtype=torch.uint8, device=acts.device)
    if costs is None:
        costs = torch.empty(N, dtype=F32, device=acts.device)
    if want_grad and grads is None:
        grads = torch.empty_like(acts)
    call(entry, ptr(acts), ptr(grads) if want_grad else None, ptr(grad_ntc_bf16), float(scale), ptr(labels),
         ptr(label_lengths), ptr(input_lengths), C, N, T, max_label_len, blank, ptr(costs), ptr(workspace), workspace.numel(), _st())
    return costs, (grads if want_grad else None)


def ctc_loss_long(acts, labels, label_lengths, input_lengths, max_label_len, blank=0, want_grad=True, grad_ntc_bf16=None, scale=1.0,
                  workspace=None, costs=None, grads=None):
    """Labels of up to 255 characters in one launch: costs, the f32 [T, N, C] gradient (want_grad) and / or scale * gradient as bf16
    [N, T, C] (grad_ntc_bf16).  -> (costs, f32 gradient or None)."""
    return _ctc_loss_tables("ocr_ctc_loss_long", ctc_long_workspace_bytes, acts, labels, label_lengths, input_lengths, max_label_len, blank,
                            want_grad, grad_ntc_bf16, scale, workspace, costs, grads)


def ctc_wide_supported(C, T, max_label_len):
    """C <= 16384 classes, labels of up to 255 characters (host arithmetic only)."""
    return bool(nat.lib().ocr_ctc_wide_supported(C, T, max_label_len))


def ctc_wide_workspace_bytes(C, max_label_len, max_time, minibatch):
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_wide_workspace_size", C, max_label_len, max_time, minibatch, ctypes.byref(sz))
    return sz.value


def ctc_loss_wide(acts, labels, label_lengths, input_lengths, max_label_len, blank=0, want_grad=True, grad_ntc_bf16=None, scale=1.0,
                  workspace=None, costs=None, grads=None):
    """Wide alphabets (up to 16384 classes) in two launches, one workgroup per logit row and one per sample: costs, the f32 [T, N, C]
    gradient (want_grad) and / or scale * gradient as bf16 [N, T, C] (grad_ntc_bf16).  -> (costs, f32 gradient or None)."""
    return _ctc_loss_tables("ocr_ctc_loss_wide", ctc_wide_workspace_bytes, acts, labels, label_lengths, input_lengths, max_label_len, blank,
                            want_grad, grad_ntc_bf16, scale, workspace, costs, grads)


def ctc_score_supported(C, T, max_label_len, K):
    """C <= 16384 classes, candidates of up to 255 characters, up to 65536 of them (host arithmetic only)."""
    return bool(nat.lib().ocr_ctc_score_supported(C, T, max_label_len, K))


def ctc_score_workspace_bytes(C, max_time, minibatch):
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_score_workspace_size", C, max_time, minibatch, ctypes.byref(sz))
    return sz.value


def ctc_score(acts, input_lengths, lexicon, lexicon_lengths, blank=0, per_sample=False, workspace=None, costs=None, want_best=True):
    """CTC costs of K candidate strings against one set of logits: acts f32 [T, N, C] unnormalised; lexicon int32 [K, Lmax] with lengths [K],
    shared by every sample, or [N, K, Lmax] with lengths [N, K] (per_sample).  -> (costs [N, K] f32, +inf for a candidate that cannot be
    emitted; best [N] i32, -1 where no candidate can; best_cost [N] f32; log_norm [N] f32 = log sum_k exp(-costs)); the last three are None
    when want_best is False."""
    T, N, C = acts.shape
    _dev(acts)
    want = 3 if per_sample else 2
    if lexicon.dim() != want or lexicon_lengths.dim() != want - 1 or tuple(lexicon.shape[:-1]) != tuple(lexicon_lengths.shape) or \
            (per_sample and lexicon.shape[0] != N):
        raise ValueError('lexicon %s / lengths %s do not fit a %s lexicon for %d samples'
                         % (tuple(lexicon.shape), tuple(lexicon_lengths.shape), 'per-sample' if per_sample else 'shared', N))
    K, Lmax = int(lexicon.shape[-2]), int(lexicon.shape[-1])
    if workspace is None:
        workspace = torch.empty(ctc_score_workspace_bytes(C, T, N), dtype=torch.uint8, device=acts.device)
    if costs is None:
        costs = torch.empty((N, K), dtype=F32, device=acts.device)
    best = best_cost = log_norm = None
    if want_best:
        best = torch.empty(N, dtype=torch.int32, device=acts.device)
        best_cost = torch.empty(N, dtype=F32, device=acts.device)
        log_norm = torch.empty(N, dtype=F32, device=acts.device)
    # (a lexicon of empty strings only has Lmax = 0 and no storage: any non-NULL address does, no word of it is read)
    call("ocr_ctc_score", ptr(acts), ptr(input_lengths), ptr(lexicon) if lexicon.numel() else ptr(lexicon_lengths), ptr(lexicon_lengths),
         K if per_sample else 0, C, N, T, K, Lmax, blank, ptr(costs), ptr(best), ptr(best_cost), ptr(log_norm), ptr(workspace),
         workspace.numel(), _st())
    return costs, best, best_cost, log_norm


def ctc_score_fuse(costs, lm_score):
    """Shallow fusion of scored candidates, in place: costs f32 [N, K] (ctc_score's) -= lm_score f32 [N, K] (ctc_beam_lm's), both contiguous.
    -> (costs, best, best_cost, log_norm) of the fused costs as ctc_score returns them; an empty slot (+inf, -inf) stays +inf."""
    _dev(costs)
    if costs.dim() != 2 or costs.shape != lm_score.shape or costs.dtype != F32 or lm_score.dtype != F32 or not costs.is_contiguous() or \
            not lm_score.is_contiguous():
        raise ValueError('ctc_score_fuse takes two contiguous float32 [N, K] matrices (got %s %s / %s %s)'
                         % (costs.dtype, tuple(costs.shape), lm_score.dtype, tuple(lm_score.shape)))
    N, K = int(costs.shape[0]), int(costs.shape[1])
    best = torch.empty(N, dtype=torch.int32, device=costs.device)
    best_cost = torch.empty(N, dtype=F32, device=costs.device)
    log_norm = torch.empty(N, dtype=F32, device=costs.device)
    call("ocr_ctc_score_fuse", ptr(costs), ptr(lm_score), N, K, ptr(best), ptr(best_cost), ptr(log_norm), _st())
    return costs, best, best_cost, log_norm


def ctc_trie_supported(C, T, K):
    """C <= 16384 classes, a lexicon of up to 1048576 words (host arithmetic only)."""
    return bool(nat.lib().ocr_ctc_trie_supported(C, T, K))


def ctc_trie_workspace_bytes(C, max_time, minibatch):
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_trie_workspace_size", C, max_time, minibatch, ctypes.byref(sz))
    return sz.value


def ctc_score_trie(acts, input_lengths, trie, workspace=None, costs=None, want_best=True):
    """ctc_score for a lexicon.LexiconTrie (one lexicon shared by the samples, its blank and class count the trie's): every node of the prefix
    tree runs its recursion once.  -> (costs [N, K] f32 in the trie's original word order, best, best_cost, log_norm) as ctc_score.  The first
    call on a device copies the trie's arrays there (trie.device_arrays(device) does it ahead of a graph capture); later calls only launch."""
    T, N, C = acts.shape
    _dev(acts)
    if C != trie.num_classes:
        raise ValueError('logits of %d classes, a LexiconTrie built for %d' % (C, trie.num_classes))
    K = trie.num_words
    arrays = trie.device_arrays(acts.device)
    if workspace is None:
        workspace = torch.empty(ctc_trie_workspace_bytes(C, T, N), dtype=torch.uint8, device=acts.device)
    if costs is None:
        costs = torch.empty((N, K), dtype=F32, device=acts.device)
    best = best_cost = log_norm = None
    if want_best:
        best = torch.empty(N, dtype=torch.int32, device=acts.device)
        best_cost = torch.empty(N, dtype=F32, device=acts.device)
        log_norm = torch.empty(N, dtype=F32, device=acts.device)
    call("ocr_ctc_score_trie", ptr(acts), ptr(input_lengths), *[ptr(a) for a in arrays], trie.num_chunks, trie.chunk_nodes, C, N, T, K, trie.blank,
         ptr(costs), ptr(best), ptr(best_cost), ptr(log_norm), ptr(workspace), workspace.numel(), _st())
    return costs, best, best_cost, log_norm


def ctc_topk_supported(K, k):
    """Rows of up to 1048576 entries, the 1 .. 64 best of each (host arithmetic only)."""
    return bool(nat.lib().ocr_ctc_topk_supported(K, k))


def ctc_topk_plan(N, K, k):
    """-> (segments, segment_len): how ctc_topk cuts a row of K entries at N samples, a workgroup per (segment, sample); host arithmetic only."""
    if not ctc_topk_supported(K, k):
        raise ValueError('ctc_topk takes 1 <= K <= 1048576 entries and 1 <= k <= 64 (got K = %d, k = %d)' % (K, k))
    segments, segment_len = ctypes.c_int(0), ctypes.c_int(0)
    call("ocr_ctc_topk_plan", N, K, k, ctypes.byref(segments), ctypes.byref(segment_len))
    return segments.value, segment_len.value


def ctc_topk_workspace_bytes(N, K, k):
    if not ctc_topk_supported(K, k):
        raise ValueError('ctc_topk takes 1 <= K <= 1048576 entries and 1 <= k <= 64 (got K = %d, k = %d)' % (K, k))
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_topk_workspace_size", N, K, k, ctypes.byref(sz))
    return sz.value


def ctc_topk(costs, k, log_norm=None, workspace=None):
    """The k smallest entries of every row of costs (f32 [N, K]; a view with a row stride is taken as it is, its columns must be contiguous) under
    the total order (cost with -0.0 == +0.0, then the lower index), ascending; +inf entries are never returned.
    -> (index [N, k] i32, cost [N, k] f32 with the entries' own bits, log_post [N, k] f32 = (-cost) - log_norm[n] or None without log_norm,
    count [N] i32); slots at and beyond count[n] hold -1 / +inf / -inf."""
    _dev(costs)
    if costs.dim() != 2 or costs.dtype != F32 or (costs.shape[1] > 1 and costs.stride(1) != 1) or (costs.shape[0] > 1 and costs.stride(0) < costs.shape[1]):
        raise ValueError('ctc_topk takes a float32 [N, K] matrix whose rows are contiguous (got %s %s, strides %s)'
                         % (costs.dtype, tuple(costs.shape), tuple(costs.stride())))
    N, K = int(costs.shape[0]), int(costs.shape[1])
    k = int(k)
    need = ctc_topk_workspace_bytes(N, K, k)               # (ValueError for a K or k outside the limits)
    ld = int(costs.stride(0)) if N > 1 else K
    if log_norm is not None and (log_norm.dtype != F32 or log_norm.numel() != N or not log_norm.is_contiguous()):
        raise ValueError('log_norm must be a contiguous float32 [N]')
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=costs.device)
    index = torch.empty((N, k), dtype=torch.int32, device=costs.device)
    cost = torch.empty((N, k), dtype=F32, device=costs.device)
    count = torch.empty(N, dtype=torch.int32, device=costs.device)
    log_post = torch.empty((N, k), dtype=F32, device=costs.device) if log_norm is not None else None
    call("ocr_ctc_topk", ptr(costs), ld, N, K, k, ptr(log_norm), ptr(index), ptr(cost), ptr(log_post), ptr(count), ptr(workspace),
         workspace.numel(), _st())
    return index, cost, log_post, count


def ctc_align_supported(C, T, max_label_len, K):
    """C <= 16384 classes, strings of up to 255 characters, up to 65536 of them per sample, any T (host arithmetic only)."""
    return bool(nat.lib().ocr_ctc_align_supported(C, T, max_label_len, K))


def ctc_align_workspace_bytes(C, max_time, minibatch, K, max_label_len):
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_align_workspace_size", C, max_time, minibatch, K, max_label_len, ctypes.byref(sz))
    return sz.value


def ctc_align(acts, input_lengths, labels, label_lengths, blank=0, shared=False, workspace=None):
    """The best (Viterbi) alignment of strings against the logits acts f32 [T, N, C] (unnormalised).  labels int32 [N, L] with lengths [N]: one
    transcript per sample; [N, K, L] with lengths [N, K]: K strings per sample; with shared=True [K, L] with lengths [K]: K strings for every
    sample.  -> (start, end: int32 [N, K, L], the first and last frame of each character; score f32 [N, K, L], the character's log-probability
    summed over its frames; path_cost f32 [N, K], minus the log-probability of the best path), the K axis squeezed for the [N, L] form.
    -1 / -1 / -inf beyond a string's length and for a string the sample cannot emit, whose path_cost is +inf."""
    T, N, C = acts.shape
    own = not shared and labels.dim() == 2
    want = 2 if (shared or own) else 3
    if labels.dim() != want or label_lengths.dim() != want - 1 or tuple(labels.shape[:-1]) != tuple(label_lengths.shape) or \
            (not shared and labels.shape[0] != N):
        raise ValueError('labels %s / lengths %s do not fit %s for %d samples'
                         % (tuple(labels.shape), tuple(label_lengths.shape), 'a shared [K, L] list' if shared else 'the [N, L] or [N, K, L] layout', N))
    _dev(acts)
    K = 1 if own else int(labels.shape[-2])
    Lmax = int(labels.shape[-1])
    if workspace is None:
        workspace = torch.empty(ctc_align_workspace_bytes(C, T, N, K, Lmax), dtype=torch.uint8, device=acts.device)
    start = torch.empty((N, K, Lmax), dtype=torch.int32, device=acts.device)
    end = torch.empty((N, K, Lmax), dtype=torch.int32, device=acts.device)
    score = torch.empty((N, K, Lmax), dtype=F32, device=acts.device)
    path_cost = torch.empty((N, K), dtype=F32, device=acts.device)
    # (strings of no characters only: Lmax = 0 and no storage; any non-NULL address does, no word of it is read or written)
    some = labels.numel() > 0
    call("ocr_ctc_align", ptr(acts), ptr(input_lengths), ptr(labels) if some else ptr(label_lengths), ptr(label_lengths), 0 if shared else K,
         C, N, T, K, Lmax, blank, ptr(start) if some else ptr(path_cost), ptr(end) if some else ptr(path_cost),
         ptr(score) if some else ptr(path_cost), ptr(path_cost), ptr(workspace), workspace.numel(), _st())
    if own:
        return start[:, 0], end[:, 0], score[:, 0], path_cost[:, 0]
    return start, end, score, path_cost


def edit_distance_supported(Ka, Kb, N):
    """Up to 65536 strings a side, 65535 samples and 2^30 pairs in all (host arithmetic only)."""
    return bool(nat.lib().ocr_edit_distance_supported(int(Ka), int(Kb), int(N)))


def _edit_operand(name, s, s_len, shared):
    """-> (K, N or None for a shared list, pitch, sample stride in ints) of one side of edit_distance, checked."""
    want = 2 if shared else s.dim()
    if s.dtype != torch.int32 or s_len.dtype != torch.int32 or s.dim() != want or s.dim() not in (2, 3) or \
            tuple(s.shape[:-1]) != tuple(s_len.shape) or not s_len.is_contiguous() or s.device != s_len.device:
        raise ValueError('%s: int32 %s strings with contiguous int32 lengths of the leading shape (got %s %s / %s %s)'
                         % (name, '[K, L] (shared)' if shared else '[N, L] or [N, K, L]', s.dtype, tuple(s.shape), s_len.dtype, tuple(s_len.shape)))
    L = int(s.shape[-1])
    if (L > 1 and s.stride(-1) != 1) or any(st < 0 for st in s.stride()):
        raise ValueError('%s: the last dimension must be contiguous and no stride negative (strides %s)' % (name, tuple(s.stride())))
    if s.shape[0] < 1 or s.shape[-2] < 1:
        raise ValueError('%s: no strings (shape %s)' % (name, tuple(s.shape)))
    K = int(s.shape[-2]) if (shared or s.dim() == 3) else 1
    rows = s.dim() == 3 or shared                       # the K axis is a dimension of the tensor: its stride is the pitch
    ld = int(s.stride(-2)) if (rows and K > 1) else L
    if ld < L:
        raise ValueError('%s: strings overlap (row stride %d below their %d columns)' % (name, ld, L))
    if shared:
        return K, None, ld, 0
    N = int(s.shape[0])
    sn = int(s.stride(0)) if N > 1 else max(K * ld, 1)
    if sn == 0:
        raise ValueError('%s: a sample stride of 0 is a shared list: pass it as [K, L] with shared_%s=True' % (name, name))
    return K, N, ld, sn


def edit_distance(a, a_len, b, b_len, ignore=None, shared_a=False, shared_b=False, want_counts=False):
    """Levenshtein distances (unit costs) of every string of a against every string of b, per sample.  Each side is int32 [N, L] with lengths
    [N] (one string per sample), [N, K, L] with lengths [N, K], or with shared_*=True [K, L] with lengths [K] for every sample; the last
    dimension contiguous, the pitches taken from the strides (a slice of the n-best paths goes in as it is).  ignore: a class dropped from both
    strings before comparing (None: nothing is).  -> dist int32 [N, Ka, Kb], -1 for every pair with a "no string" (a length below 0 or above
    the pitch, or more than 255 characters counted); with want_counts also (a_count, b_count), int32 shaped like the lengths: the counted
    lengths, -1 for "no string"."""
    Ka, Na, a_ld, a_sn = _edit_operand('a', a, a_len, shared_a)
    Kb, Nb, b_ld, b_sn = _edit_operand('b', b, b_len, shared_b)
    if Na is not None and Nb is not None and Na != Nb:
        raise ValueError('a holds %d samples, b %d' % (Na, Nb))
    N = Na if Na is not None else Nb if Nb is not None else 1
    if not edit_distance_supported(Ka, Kb, N):
        raise ValueError('edit_distance takes 1 <= N <= 65535, 1 <= Ka, Kb <= 65536 and N * Ka * Kb <= 2^30 (got N = %d, Ka = %d, Kb = %d)' % (N, Ka, Kb))
    _dev(a)
    _dev(b)
    dist = torch.empty((N, Ka, Kb), dtype=torch.int32, device=a.device)
    a_count = torch.empty_like(a_len) if want_counts else None
    b_count = torch.empty_like(b_len) if want_counts else None
    # (strings of no columns have no storage: any non-NULL address does, no word of it is read)
    call("ocr_edit_distance", ptr(a) if a.numel() else ptr(a_len), ptr(a_len), a_ld, a_sn, Ka, ptr(b) if b.numel() else ptr(b_len), ptr(b_len),
         b_ld, b_sn, Kb, N, -1 if ignore is None else int(ignore), ptr(dist), ptr(a_count), ptr(b_count), _st())
    return (dist, a_count, b_count) if want_counts else dist


def edit_stats(dist, ref_count):
    """-> int64 [4] on the device: {sum of dist, sum of ref_count, number with dist == 0, number counted} over the pairs with dist >= 0;
    dist and ref_count contiguous int32 of the same number of elements (ref_count: the reference's counted length of each pair)."""
    if dist.dtype != torch.int32 or ref_count.dtype != torch.int32 or dist.numel() != ref_count.numel() or dist.numel() < 1 or \
            not dist.is_contiguous() or not ref_count.is_contiguous():
        raise ValueError('edit_stats takes contiguous int32 dist and ref_count of one size (got %s %s / %s %s)'
                         % (dist.dtype, tuple(dist.shape), ref_count.dtype, tuple(ref_count.shape)))
    _dev(dist)
    stats = torch.empty(4, dtype=torch.int64, device=dist.device)
    call("ocr_edit_stats", ptr(dist), ptr(ref_count), dist.numel(), ptr(stats), _st())
    return stats


MBR_MAX_K = 128


def mbr_select(dist, costs):
    """Minimum-Bayes-risk selection: dist int32 [N, K, K], costs f32 [N, K] (minus log-probabilities), both contiguous, K <= 128.
    -> (risk f32 [N, K], the expected distance of each candidate to the others under their posterior within the list, +inf for a candidate
    that is not valid (cost not finite or dist[n, i, i] < 0); best int32 [N], the arg-min under (risk, cost, index), -1 where none is valid;
    best_risk f32 [N])."""
    if dist.dim() != 3 or costs.dim() != 2 or dist.dtype != torch.int32 or costs.dtype != F32 or dist.shape[1] != dist.shape[2] or \
            tuple(dist.shape[:2]) != tuple(costs.shape) or not dist.is_contiguous() or not costs.is_contiguous():
        raise ValueError('mbr_select takes contiguous int32 dist [N, K, K] and float32 costs [N, K] (got %s %s / %s %s)'
                         % (dist.dtype, tuple(dist.shape), costs.dtype, tuple(costs.shape)))
    N, K = int(costs.shape[0]), int(costs.shape[1])
    if not (1 <= K <= MBR_MAX_K and 1 <= N <= 65535):
        raise ValueError('mbr_select takes 1 <= K <= %d candidates of 1 <= N <= 65535 samples (got K = %d, N = %d)' % (MBR_MAX_K, K, N))
    _dev(dist)
    risk = torch.empty((N, K), dtype=F32, device=dist.device)
    best = torch.empty(N, dtype=torch.int32, device=dist.device)
    best_risk = torch.empty(N, dtype=F32, device=dist.device)
    call("ocr_mbr_select", ptr(dist), ptr(costs), N, K, ptr(risk), ptr(best), ptr(best_risk), _st())
    return risk, best, best_risk


def ctc_greedy_decode(acts, input_lengths, blank=0, pad_value=0):
    T, N, C = acts.shape
    out = torch.empty((N, T), dtype=torch.int32, device=acts.device)
    lens = torch.empty(N, dtype=torch.int32, device=acts.device)
    call("ocr_ctc_greedy_decode", ptr(_dev(acts)), ptr(input_lengths), C, N, T, blank, pad_value, ptr(out), ptr(lens), _st())
    return out, lens


def ctc_beam_decode(acts, input_lengths, beam_width=100, merge_repeated=True, pad_value=0, workspace=None):
    """tf.nn.ctc_beam_search_decoder semantics (blank = C-1).  Returns (dense [N, T] int32, lengths, neg_log_prob)."""
    T, N, C = acts.shape
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_beam_workspace_size", C, N, T, beam_width, ctypes.byref(sz))
    if workspace is None or workspace.numel() < sz.value:
        workspace = torch.empty(sz.value, dtype=torch.uint8, device=acts.device)
    out = torch.empty((N, T), dtype=torch.int32, device=acts.device)
    lens = torch.empty(N, dtype=torch.int32, device=acts.device)
    nlp = torch.empty(N, dtype=F32, device=acts.device)
    call("ocr_ctc_beam_decode", ptr(_dev(acts)), ptr(input_lengths), C, N, T, beam_width, int(merge_repeated), pad_value,
         ptr(out), ptr(lens), ptr(nlp), ptr(workspace), workspace.numel(), _st())
    return out, lens, nlp


def ctc_beam_nbest(acts, input_lengths, top_paths, beam_width=100, blank=None, merge_repeated=False, pad_value=0, workspace=None):
    """The top_paths best prefixes of the beam search, best first, with any class as the blank (None: C - 1, TF's).  blank=0 with
    merge_repeated=False is the textbook CTC prefix search, whose costs compare with ctc_score(blank=0).
    -> (paths [N, top_paths, T] int32, lengths [N, top_paths] int32, neg_log_prob [N, top_paths] f32, count [N] int32); slots at and beyond
    count[n] hold pad_value / -1 / +inf."""
    T, N, C = acts.shape
    blank = C - 1 if blank is None else int(blank)
    top_paths = int(top_paths)
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_beam_workspace_size", C, N, T, beam_width, ctypes.byref(sz))
    if workspace is None or workspace.numel() < sz.value:
        workspace = torch.empty(sz.value, dtype=torch.uint8, device=acts.device)
    shape = (N, max(top_paths, 0))                 # (a top_paths outside the limits is the entry's to refuse)
    paths = torch.empty(shape + (T,), dtype=torch.int32, device=acts.device)
    lens = torch.empty(shape, dtype=torch.int32, device=acts.device)
    nlp = torch.empty(shape, dtype=F32, device=acts.device)
    count = torch.empty(N, dtype=torch.int32, device=acts.device)
    call("ocr_ctc_beam_decode_nbest", ptr(_dev(acts)), ptr(input_lengths), C, N, T, beam_width, top_paths, blank, int(merge_repeated),
         pad_value, ptr(paths), ptr(lens), ptr(nlp), ptr(count), ptr(workspace), workspace.numel(), _st())
    return paths, lens, nlp, count


def ctc_beam_lm_supported(C, K, H):
    """Whether ctc_beam_lm covers C classes at beam width K with an automaton of H states (host arithmetic only): K <= 128, H <= 1048576 and
    the table kernel's LDS with two more beam arrays, which at K = 100 ends at 256 classes."""
    return bool(nat.lib().ocr_ctc_beam_lm_supported(int(C), int(K), int(H)))


def ctc_beam_lm(acts, input_lengths, automaton, top_paths, beam_width=100, blank=0, pad_value=0, workspace=None):
    """The prefix search of ctc_beam_nbest (merge_repeated=False) fused with an automaton.LabelAutomaton over the caller's class ids: every
    extension of a prefix also pays the automaton's weight, forbidden transitions are never taken, and the final ranking adds the end weight
    of the prefix's state.  -> (paths [N, top_paths, T] int32, lengths [N, top_paths] int32, neg_log_prob [N, top_paths] f32 = minus the fused
    score, lm_score [N, top_paths] f32 = the automaton's share of it (automaton.score(labels)), count [N] int32); slots at and beyond
    count[n] hold pad_value / -1 / +inf / -inf.  -neg_log_prob - lm_score is the beam's acoustic log-probability of the string."""
    T, N, C = acts.shape
    _dev(acts)
    if automaton.num_classes != C:
        raise ValueError('logits of %d classes, a LabelAutomaton built for %d' % (C, automaton.num_classes))
    top_paths, blank = int(top_paths), int(blank)
    if 0 <= blank < C and automaton.blank != blank:              # (a blank outside the alphabet is the entry's to refuse)
        raise ValueError('blank %d, but the LabelAutomaton was built with blank %d' % (blank, automaton.blank))
    nxt, weight, final = automaton.device_arrays(acts.device)
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_beam_lm_workspace_size", C, N, T, beam_width, ctypes.byref(sz))
    if workspace is None or workspace.numel() < sz.value:
        workspace = torch.empty(sz.value, dtype=torch.uint8, device=acts.device)
    shape = (N, max(top_paths, 0))                 # (a top_paths outside the limits is the entry's to refuse)
    paths = torch.empty(shape + (T,), dtype=torch.int32, device=acts.device)
    lens = torch.empty(shape, dtype=torch.int32, device=acts.device)
    nlp = torch.empty(shape, dtype=F32, device=acts.device)
    lm_score = torch.empty(shape, dtype=F32, device=acts.device)
    count = torch.empty(N, dtype=torch.int32, device=acts.device)
    call("ocr_ctc_beam_decode_lm", ptr(acts), ptr(input_lengths), C, N, T, beam_width, top_paths, blank, pad_value, ptr(nxt), ptr(weight),
         ptr(final), automaton.num_states, ptr(paths), ptr(lens), ptr(nlp), ptr(lm_score), ptr(count), ptr(workspace), workspace.numel(), _st())
    return paths, lens, nlp, lm_score, count


def ctc_beam_lm_sparse_supported(C, K, cutoff, H, A):
    """Whether ctc_beam_lm_sparse covers C classes at beam width K and class cutoff `cutoff` with an automaton of H states and A arcs (host
    arithmetic only): 2 <= C <= 16384, K <= 128, 1 <= cutoff <= K + 1, H <= 1 << 24, A <= 1 << 28."""
    return bool(nat.lib().ocr_ctc_beam_lm_sparse_supported(int(C), int(K), int(cutoff), int(H), int(A)))


def ctc_beam_lm_sparse(acts, input_lengths, automaton, top_paths, beam_width=100, cutoff=None, blank=0, pad_value=0, workspace=None):
    """ctc_beam_lm for wide alphabets (up to 16384 classes): the search runs on the wide kernel and reads an automaton.SparseLabelAutomaton,
    whose failure arcs are followed on the device.  New children of a frame come from its min(cutoff, C - 1) likeliest non-blank classes
    (None: beam_width + 1); with weights in the search that acoustic pruning is part of the result.  Outputs as ctc_beam_lm's."""
    T, N, C = acts.shape
    _dev(acts)
    if automaton.num_classes != C:
        raise ValueError('logits of %d classes, a SparseLabelAutomaton built for %d' % (C, automaton.num_classes))
    top_paths, blank = int(top_paths), int(blank)
    cutoff = int(beam_width) + 1 if cutoff is None else int(cutoff)
    if 0 <= blank < C and automaton.blank != blank:              # (a blank outside the alphabet is the entry's to refuse)
        raise ValueError('blank %d, but the SparseLabelAutomaton was built with blank %d' % (blank, automaton.blank))
    arrays = automaton.device_arrays(acts.device)
    sz = ctypes.c_size_t(0)
    call("ocr_ctc_beam_lm_sparse_workspace_size", C, N, T, beam_width, ctypes.byref(sz))
    if workspace is None or workspace.numel() < sz.value:
        workspace = torch.empty(sz.value, dtype=torch.uint8, device=acts.device)
    shape = (N, max(top_paths, 0))                 # (a top_paths outside the limits is the entry's to refuse)
    paths = torch.empty(shape + (T,), dtype=torch.int32, device=acts.device)
    lens = torch.empty(shape, dtype=torch.int32, device=acts.device)
    nlp = torch.empty(shape, dtype=F32, device=acts.device)
    lm_score = torch.empty(shape, dtype=F32, device=acts.device)
    count = torch.empty(N, dtype=torch.int32, device=acts.device)
    call("ocr_ctc_beam_decode_lm_sparse", ptr(acts), ptr(input_lengths), C, N, T, beam_width, cutoff, top_paths, blank, pad_value,
         *[ptr(v) for v in arrays], automaton.num_states, automaton.num_arcs, ptr(paths), ptr(lens), ptr(nlp), ptr(lm_score), ptr(count),
         ptr(workspace), workspace.numel(), _st())
    return paths, lens, nlp, lm_score, count


BEAM_KERNEL_NAMES = (None, "table", "wide")


def ctc_beam_kernel_choice(alphabet_size, beam_width):
    """'table' / 'wide': the kernel ctc_beam_decode runs at this shape under the current engine; None where it refuses (host-only query)."""
    return BEAM_KERNEL_NAMES[nat.lib().ocr_ctc_beam_kernel_choice(int(alphabet_size), int(beam_width))]


def set_beam_engine(engine):
    """0 (default): table kernel where it fits, wide kernel elsewhere; 2: wide kernel wherever it covers the shape."""
    call("ocr_set_beam_engine", int(engine))


# ----------------------------------------------------------------------------------------------- GEMMs
def gemm_nt(P, Q, out=None, *, M=None, N=None, K=None, ldp=None, ldq=None, ldo=None, bias=None, relu=False,
            out_f32=False, mask=None, accumulate=False, splits=1, row_group=0, row_skip=0, rowswap=None):
    """out[m][n] = sum_k P[m][k] Q[n][k]; P, Q bf16 (K contiguous)."""
    M = P.shape[0] if M is None else M
    K = P.shape[1] if K is None else K
    N = Q.shape[0] if N is None else N
    ldp = P.stride(0) if ldp is None else ldp
    ldq = Q.stride(0) if ldq is None else ldq
    if out is None:
        out = torch.empty((M, N), dtype=F32 if out_f32 else BF16, device=P.device)
    ldo = out.stride(0) if ldo is None else ldo
    flags = 0
    if bias is not None: flags |= EPI_BIAS
    if relu: flags |= EPI_RELU
    if out.dtype == F32: flags |= EPI_OUT_F32
    if mask is not None: flags |= EPI_MASK
    if accumulate: flags |= EPI_ACCUM
    si = so = 0
    if rowswap is not None:
        flags |= EPI_ROWSWAP
        si, so = rowswap
    call("ocr_gemm_nt_bf16", ptr(_dev(P)), ldp, ptr(Q), ldq, ptr(out), ldo, M, N, K, ptr(bias), ptr(mask),
         mask.stride(0) if mask is not None else 0, flags, splits, row_group, row_skip, si, so, _st())
    return out


CONV_KERNEL_NAMES = ("gemm", "conv_halo", "conv_k2/A", "conv_k2/D", "conv_k3/A", "conv_k3/D", "conv_k3w/A", "conv_k3w/D", "conv_ws")


def conv3x3_kernel_choice(Nb, W, H, Cin, Cout, *, bias=True, relu=True, mask=False, accumulate=False, pool=(0, 0)):
    """Name of the kernel family ocr_conv3x3_bf16 / ocr_conv3x3_relu_pool_bf16 take for this shape (host-only query, no GPU needed)."""
    flags = (nat.EPI_BIAS if bias else 0) | (nat.EPI_RELU if relu else 0) | (nat.EPI_MASK if mask else 0) | (nat.EPI_ACCUM if accumulate else 0)
    rc = nat.lib().ocr_conv3x3_kernel_choice(int(Nb), int(W), int(H), int(Cin), int(Cout), flags, int(pool[0]), int(pool[1]))
    if rc < 0:
        raise nat.NativeError("ocr_conv3x3_kernel_choice failed: status %d (%s)" % (-rc, nat.status_string(-rc)))
    return CONV_KERNEL_NAMES[rc]


def conv3x3_accum_supported(Nb, W, H, Cin, Cout):
    return bool(nat.lib().ocr_conv3x3_accum_supported(Nb, W, H, Cin, Cout))


def conv3x3(x, wpack, out=None, *, bias=None, relu=False, mask=None, accumulate=False):
    """x bf16 [Nb, W, H, Cin]; wpack bf16 [Cout, 3, 3, Cin] -> bf16 [Nb, W, H, Cout]  (accumulate: out += result)."""
    Nb, W, H, Cin = x.shape
    Cout = wpack.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty((Nb, W, H, Cout), dtype=BF16, device=x.device)
    flags = ((EPI_BIAS if bias is not None else 0) | (EPI_RELU if relu else 0) | (EPI_MASK if mask is not None else 0) |
             (EPI_ACCUM if accumulate else 0))
    call("ocr_conv3x3_bf16", ptr(_dev(x)), ptr(wpack), ptr(out), Nb, W, H, Cin, Cout, ptr(bias), ptr(mask), flags, _st())
    return out


def conv3x3_pool_supported(Nb, W, H, Cin, Cout, kw, kh):
    return bool(nat.lib().ocr_conv3x3_pool_supported(Nb, W, H, Cin, Cout, kw, kh))


def conv3x3_relu_pool(x, wpack, out, pooled, bias, kw, kh):
    """out = relu(conv3x3(x) + bias) and pooled = max_pool(out, window (kw along W, kh along H)) from one launch."""
    Nb, W, H, Cin = x.shape
    call("ocr_conv3x3_relu_pool_bf16", ptr(_dev(x)), ptr(wpack), ptr(out), ptr(pooled), Nb, W, H, Cin, wpack.shape[0], ptr(bias),
         kw, kh, _st())
    return out, pooled


def conv3x3_pool_codes_supported(Nb, W, H, Cin, Cout, kw, kh):
    """Whether the kernel planned for this shape's conv3x3_relu_pool can also write the pool's routing codes (conv3x3_relu_pool_codes)."""
    return bool(nat.lib().ocr_conv3x3_pool_codes_supported(Nb, W, H, Cin, Cout, kw, kh))


def conv3x3_relu_pool_codes(x, wpack, out, pooled, codes, bias, kw, kh):
    """conv3x3_relu_pool that also writes the pool's routing codes (int32 [Nb * W/kw * H/kh, Cout / 8], what maxpool_bwd_codes reads).  out may be
    None: the full-resolution tensor is then not stored at all."""
    Nb, W, H, Cin = x.shape
    Cout = wpack.shape[0]
    assert codes.dtype == torch.int32 and codes.numel() == Nb * (W // kw) * (H // kh) * (Cout // 8), (codes.dtype, tuple(codes.shape))
    call("ocr_conv3x3_relu_pool_codes_bf16", ptr(_dev(x)), ptr(wpack), ptr(out), ptr(pooled), ptr(codes), Nb, W, H, Cin, Cout, ptr(bias),
         kw, kh, _st())
    return out, pooled, codes


def conv3x3_unpool_supported(Nb, W, H, Cin, Cout, kw, kh):
    """Whether conv3x3_dgrad_unpool has an instance for this data gradient ((Nb, W, H): the POOLED resolution; host-only query)."""
    return bool(nat.lib().ocr_conv3x3_unpool_supported(int(Nb), int(W), int(H), int(Cin), int(Cout), int(kw), int(kh)))


def conv3x3_dgrad_unpool(dy, wdgrad, codes, kw, kh, relu_mask, out=None):
    """The data gradient conv3x3(dy, wdgrad) of a convolution behind a max-pool, scattered to the pool's input resolution by the routing codes
    in the kernel's write-out: bit-identical to maxpool_bwd_codes(codes, conv3x3(dy, wdgrad), kw, kh, relu_mask) where conv3x3 runs an
    aligned-width conv_k3 kernel; the pooled gradient itself is not stored.  dy bf16 [Nb, W, H, Cin], wdgrad bf16 [Cout, 3, 3, Cin],
    codes int32 [Nb * W * H, Cout / 8] -> bf16 [Nb, W * kw, H * kh, Cout]."""
    Nb, W, H, Cin = dy.shape
    Cout = wdgrad.shape[0]
    assert codes.dtype == torch.int32 and codes.numel() == Nb * W * H * (Cout // 8), (codes.dtype, tuple(codes.shape))
    if out is None:
        out = torch.empty((Nb, W * kw, H * kh, Cout), dtype=BF16, device=dy.device)
    assert out.numel() == Nb * W * kw * H * kh * Cout
    call("ocr_conv3x3_dgrad_unpool_bf16", ptr(_dev(dy)), ptr(wdgrad), ptr(out), ptr(codes), Nb, W, H, Cin, Cout, kw, kh, int(relu_mask),
         _st())
    return out


def gemm_tn(A, B, out, *, Mk=None, I=None, J=None, lda=None, ldb=None, ldo=None, row_group=0, row_skip=0,
            a_row_off=0, scale=1.0, splits=0, colsum=None):
    """out[I][J] (f32) += scale * A^T B;  colsum[J] += scale * column sums of B (bias gradient) when given."""
    Mk = B.shape[0] if Mk is None else Mk
    I = A.shape[1] if I is None else I
    J = B.shape[1] if J is None else J
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    ldo = out.stride(0) if ldo is None else ldo
    call("ocr_gemm_tn_bf16", ptr(_dev(A)), lda, ptr(B), ldb, ptr(out), ldo, Mk, I, J, row_group, row_skip, a_row_off,
         float(scale), splits, ptr(colsum), _st())
    return out


def gemm_tn_split_workspace(Mk, I, J):
    """float32 elements of the workspace gemm_tn_split needs for this shape."""
    n = nat.lib().ocr_gemm_tn_split_workspace_floats(int(Mk), int(I), int(J))
    if n < 0:
        raise nat.NativeError("ocr_gemm_tn_split_workspace_floats: invalid shape (%d, %d, %d)" % (Mk, I, J))
    return int(n)


def gemm_tn_split(A, B, out, ws, *, colsum=None, scale=1.0):
    """out[I][J] (f32) += scale * A^T B and colsum[J] += scale * column sums of B, like gemm_tn on plain rows, but reproducible bit for bit:
    the splits of the contraction go through the float32 workspace `ws` (gemm_tn_split_workspace elements) and are added in a fixed order."""
    Mk, I, J = B.shape[0], A.shape[1], B.shape[1]
    call("ocr_gemm_tn_split_bf16", ptr(_dev(A)), A.stride(0), ptr(B), B.stride(0), ptr(out), out.stride(0), Mk, I, J, float(scale),
         ptr(colsum), ptr(ws), ws.numel(), _st())
    return out


def gemm_tn_batched(A, lda, strideA, B, ldb, strideB, out, ldo, strideOut, Mk, I, J, nbatch, colsum=None, strideColsum=0,
                    scale=1.0, splits=0):
    """nbatch independent out_b[I][J] += scale * A_b^T B_b in one launch (element strides between the problems)."""
    call("ocr_gemm_tn_batched_bf16", ptr(_dev(A)), lda, strideA, ptr(B), ldb, strideB, ptr(out), ldo, strideOut, Mk, I, J, nbatch,
         float(scale), splits, ptr(colsum), strideColsum, _st())
    return out


class TnJob(ctypes.Structure):
    """ocr_tn_job (include/ocr_hip.h): one batched product out_b[I][J] += scale * A_b^T B_b (+ column sums of B_b) of ocr_gemm_tn_jobs_bf16."""
    _fields_ = [("A", ctypes.c_void_p), ("lda", ctypes.c_long), ("strideA", ctypes.c_long),
                ("B", ctypes.c_void_p), ("ldb", ctypes.c_long), ("strideB", ctypes.c_long),
                ("out", ctypes.c_void_p), ("ldo", ctypes.c_long), ("strideOut", ctypes.c_long),
                ("colsum", ctypes.c_void_p), ("strideColsum", ctypes.c_long),
                ("Mk", ctypes.c_int), ("I", ctypes.c_int), ("J", ctypes.c_int), ("nbatch", ctypes.c_int),
                ("row_group", ctypes.c_int), ("row_skip", ctypes.c_int), ("scale", ctypes.c_float), ("reserved", ctypes.c_int)]


def tn_job(A, lda, B, ldb, out, ldo, Mk, I, J, *, nbatch=1, strideA=0, strideB=0, strideOut=0, colsum=None, strideColsum=0, row_group=0,
           row_skip=0, scale=1.0):
    """Descriptor of a plain weight-gradient product for gemm_tn_jobs (the tensors must stay alive and untouched until the launch)."""
    return TnJob(ptr(_dev(A)), lda, strideA, ptr(_dev(B)), ldb, strideB, ptr(out), ldo, strideOut, ptr(colsum), strideColsum,
                 Mk, I, J, nbatch, row_group, row_skip, float(scale), 0)


def gemm_tn_jobs_supported(jobs):
    arr = (TnJob * len(jobs))(*jobs)
    return bool(nat.lib().ocr_gemm_tn_jobs_supported(ctypes.cast(arr, ctypes.c_void_p), len(jobs)))


def gemm_tn_jobs(jobs):
    """1 or 2 products in ONE launch of the ping-pong kernel (no split over the contraction, no atomics)."""
    arr = (TnJob * len(jobs))(*jobs)
    call("ocr_gemm_tn_jobs_bf16", ctypes.cast(arr, ctypes.c_void_p), len(jobs), _st())


def gemm_tn_jobs_nt_supported(jobs, M, N, K, flags=0):
    """Whether gemm_tn_jobs_nt takes these two products with an M x N x K plain GEMM of these epilogue flags in one launch (host-only query:
    the library's policy — two covered jobs whose tiles leave a quarter of the CUs free, a GEMM of the 256 x 128-tile instance)."""
    arr = (TnJob * len(jobs))(*jobs)
    return bool(nat.lib().ocr_gemm_tn_jobs_nt_supported(ctypes.cast(arr, ctypes.c_void_p), len(jobs), int(M), int(N), int(K), int(flags)))


def gemm_tn_jobs_nt(jobs, P, Q, out, *, M=None, N=None, K=None, ldp=None, ldq=None, ldo=None, row_group=0, row_skip=0):
    """gemm_tn_jobs(jobs) and gemm_nt(P, Q, out, ...) in ONE launch, bit for bit: the GEMM's workgroups run on the CUs the products' tiles
    leave idle.  Neither part may read what the other writes.  Only where gemm_tn_jobs_nt_supported says so."""
    M = P.shape[0] if M is None else M
    K = P.shape[1] if K is None else K
    N = Q.shape[0] if N is None else N
    ldp = P.stride(0) if ldp is None else ldp
    ldq = Q.stride(0) if ldq is None else ldq
    ldo = out.stride(0) if ldo is None else ldo
    arr = (TnJob * len(jobs))(*jobs)
    call("ocr_gemm_tn_jobs_nt_bf16", ctypes.cast(arr, ctypes.c_void_p), len(jobs), ptr(_dev(P)), ldp, ptr(Q), ldq, ptr(out), ldo, M, N, K,
         None, None, 0, EPI_OUT_F32 if out.dtype == F32 else 0, row_group, row_skip, 0, 0, _st())
    return out


def lstm_xh(x2d, hout, seq_len, xh, Nb, T, D, U, ndir=2):
    call("ocr_lstm_xh", ptr(_dev(x2d)), ptr(hout), ptr(seq_len), ptr(xh), Nb, T, D, U, ndir, _st())
    return xh


def conv3x3_wgrad_workspace_bytes(Nb, W, H, Cin, Cout):
    """Scratch bytes of the slab (atomic-free, deterministic) weight-gradient kernel; 0 when the shape is not covered."""
    sz = ctypes.c_size_t(0)
    call("ocr_conv3x3_wgrad_workspace_size", Nb, W, H, Cin, Cout, ctypes.byref(sz))
    return sz.value


WGRAD_KERNEL_NAMES = ("wgrad9", "wgrad9p<4>", "wgrad9p<8>", "wgrad9p<4>/zero-row", "wgrad9p<8>/zero-row", "gemm_tn2/nine-tap",
                      "gemm_tn2/paired-tap", "gemm_tn<1,4,4>", "gemm_tn<1,2,2>")


def conv3x3_wgrad_kernel_choice(Nb, W, H, Cin, Cout, *, workspace=True, splits=0):
    """(kernel name, split count S) of the 3x3 weight gradient for this shape (host-only query, no GPU needed): what conv3x3_wgrad /
    conv3x3_wgrad_deferred run with a workspace of conv3x3_wgrad_workspace_bytes (workspace=True) or without one, under the current
    wgrad engine and knobs.  S = slabs of the slab kernels, splits of the pixel contraction (atomics) of the others."""
    rc = nat.lib().ocr_conv3x3_wgrad_kernel_choice(int(Nb), int(W), int(H), int(Cin), int(Cout), int(bool(workspace)), int(splits))
    if rc < 0:
        raise nat.NativeError("ocr_conv3x3_wgrad_kernel_choice failed: status %d (%s)" % (-rc, nat.status_string(-rc)))
    return WGRAD_KERNEL_NAMES[rc & 255], rc >> 8


def conv3x3_wgrad(x, dy, dw, splits=0, dbias=None, workspace=None):
    """dw [3,3,Cin,Cout] f32 += weight gradient; dbias += column sums of dy.  With `workspace` (uint8 tensor of at least
    conv3x3_wgrad_workspace_bytes) the nine-tap slab kernel runs where it applies."""
    Nb, W, H, Cin = x.shape
    Cout = dy.shape[-1]
    if workspace is not None:
        call("ocr_conv3x3_wgrad_ws_bf16", ptr(_dev(x)), ptr(dy), ptr(dw), ptr(dbias), Nb, W, H, Cin, Cout, splits,
             ptr(workspace), workspace.numel(), _st())
    else:
        call("ocr_conv3x3_wgrad_bf16", ptr(_dev(x)), ptr(dy), ptr(dw), ptr(dbias), Nb, W, H, Cin, Cout, splits, _st())
    return dw


def conv3x3_wgrad_deferred(x, dy, dw, dbias, workspace):
    """The slab kernel only; the reduction dw += sum of the slabs (and dbias) is left to wgrad9_reduce_jobs at the end of the backward
    pass.  Returns (job, nblocks): `job` = the 64 bytes describing the pending reduction (struct W9ReduceJob) — or None when the shape
    is not covered and the whole weight gradient was computed at once.  `workspace` must not be touched until the jobs have run."""
    Nb, W, H, Cin = x.shape
    Cout = dy.shape[-1]
    job = (ctypes.c_ubyte * 64)()
    nblk, deferred = ctypes.c_int(0), ctypes.c_int(0)
    call("ocr_conv3x3_wgrad_defer_bf16", ptr(_dev(x)), ptr(dy), ptr(dw), ptr(dbias), Nb, W, H, Cin, Cout, ptr(workspace),
         workspace.numel(), ctypes.cast(job, ctypes.c_void_p), ctypes.byref(nblk), ctypes.byref(deferred), _st())
    return (bytes(job), nblk.value) if deferred.value else (None, 0)


def conv3x3_wgrad_pair_supported(shape_first, shape_second):
    """May the slab kernels of two layers, shapes (Nb, W, H, Cin, Cout), run as ONE launch with the first layer's workgroups in front
    (host-only query, no GPU needed)?  The library's whole pairing policy: both take a slab kernel, a paired instance exists, and the first
    layer's grid fills at most half the CUs."""
    a, b = (ctypes.c_int * 5)(*[int(v) for v in shape_first]), (ctypes.c_int * 5)(*[int(v) for v in shape_second])
    rc = nat.lib().ocr_conv3x3_wgrad_pair_supported(a, b)
    if rc < 0:
        raise nat.NativeError("ocr_conv3x3_wgrad_pair_supported failed: status %d (%s)" % (-rc, nat.status_string(-rc)))
    return bool(rc)


def conv3x3_wgrad_pair_deferred(first, second):
    """conv3x3_wgrad_deferred of two layers in ONE launch; `first` / `second` = (x, dy, dw, dbias, workspace) of a pair that
    conv3x3_wgrad_pair_supported accepts.  Returns ((job, nblocks), (job, nblocks)): what the two single launches would have returned —
    same split counts, same slabs."""
    args, outs = [], []
    for x, dy, dw, dbias, workspace in (first, second):
        Nb, W, H, Cin = x.shape
        shape = (ctypes.c_int * 5)(Nb, W, H, Cin, dy.shape[-1])
        args += [ptr(_dev(x)), ptr(dy), ptr(dw), ptr(dbias), shape, ptr(workspace), workspace.numel()]
        outs.append(((ctypes.c_ubyte * 64)(), ctypes.c_int(0)))
    call("ocr_conv3x3_wgrad_pair_defer_bf16", *args, ctypes.cast(outs[0][0], ctypes.c_void_p), ctypes.cast(outs[1][0], ctypes.c_void_p),
         ctypes.byref(outs[0][1]), ctypes.byref(outs[1][1]), _st())
    return tuple((bytes(job), nblk.value) for job, nblk in outs)


def wgrad9_reduce_jobs(table, njobs, total_blocks):
    call("ocr_wgrad9_reduce_jobs", ptr(_dev(table)), njobs, total_blocks, _st())


# ----------------------------------------------------------------------------------------------- HBM-bound layers
def conv1_fwd(x, w, bias, relu=True, out=None):
    Nb, W, H = x.shape
    Cout = w.shape[-1]
    if out is None:
        out = torch.empty((Nb, W, H, Cout), dtype=BF16, device=x.device)
    call("ocr_conv1_fwd", ptr(_dev(x)), ptr(w), ptr(bias), ptr(out), Nb, W, H, Cout, int(relu), _st())
    return out


def conv1_wgrad(x, dz, dw, db):
    Nb, W, H = x.shape
    call("ocr_conv1_wgrad", ptr(_dev(x)), ptr(dz), ptr(dw), ptr(db), Nb, W, H, dz.shape[-1], _st())


def eltwise(op, a, b, out):
    """op 0: out = a + b ; 1: out = relu(a) ; 2: out = (b > 0) ? a : 0 ; 3: out = relu(a + b) ; 4: out += (b > 0) ? a : 0
    (bf16, numel % 8 == 0)"""
    call("ocr_eltwise_bf16", op, ptr(_dev(a)), ptr(b), ptr(out), a.numel(), _st())
    return out


def conv1_pool_fwd(x, w, bias, out=None, zero=None, codes=None, ones=None):
    """zero (fp32 tensor, numel % 4 == 0): cleared by the same launch (the step's flat gradient buffer).  codes (int32 [Nb * W/2 * H/2, 8]):
    receives the pool routing + ReLU bits for conv1_pool_bwd(codes=...).  ones (int32 tensor, numel % 4 == 0): set to 0xFFFFFFFF by the
    same launch (the hand-off blocks of the step's persistent LSTM launches, lstm_*_seq(prepared=True))."""
    Nb, W, H = x.shape
    Cout = w.shape[-1]
    if out is None:
        out = torch.empty((Nb, W // 2, H // 2, Cout), dtype=BF16, device=x.device)
    if zero is not None or codes is not None or ones is not None:
        call("ocr_conv1_pool_fwd_train", ptr(_dev(x)), ptr(w), ptr(bias), ptr(out), Nb, W, H, Cout, ptr(codes),
             ptr(_dev(zero)) if zero is not None else None, 0 if zero is None else zero.numel(),
             ptr(_dev(ones)) if ones is not None else None, 0 if ones is None else ones.numel(), _st())
    else:
        call("ocr_conv1_pool_fwd", ptr(_dev(x)), ptr(w), ptr(bias), ptr(out), Nb, W, H, Cout, _st())
    return out


def conv1_pool_bwd(x, w, bias, dp, dw, db, codes=None):
    """codes: what conv1_pool_fwd(codes=...) saved — the gradient is routed with them (bit-identical) instead of recomputing the windows."""
    Nb, W, H = x.shape
    if codes is not None:
        call("ocr_conv1_pool_bwd_codes", ptr(_dev(x)), ptr(w), ptr(bias), ptr(dp), ptr(dw), ptr(db), Nb, W, H, w.shape[-1], ptr(codes), _st())
    else:
        call("ocr_conv1_pool_bwd", ptr(_dev(x)), ptr(w), ptr(bias), ptr(dp), ptr(dw), ptr(db), Nb, W, H, w.shape[-1], _st())


def conv1_pool_bwd_slab_rows(Nb, W, H):
    return int(nat.lib().ocr_conv1_pool_bwd_slab_rows(int(Nb), int(W), int(H)))


def conv1_pool_bwd_slab(x, w, bias, dp, slab, codes=None):
    """No atomics: block b's partial sums {dW [9][64] | db [64]} go to slab[b] (fp32 [rows, 640]); wgrad9_reduce_jobs adds the rows."""
    Nb, W, H = x.shape
    assert slab.dtype == torch.float32 and tuple(slab.shape) == (conv1_pool_bwd_slab_rows(Nb, W, H), 640)
    call("ocr_conv1_pool_bwd_slab", ptr(_dev(x)), ptr(w), ptr(bias), ptr(dp), Nb, W, H, w.shape[-1], ptr(codes), ptr(slab), _st())


def maxpool_fwd(x, kw, kh, out=None):
    Nb, W, H, C = x.shape
    if out is None:
        out = torch.empty((Nb, W // kw, H // kh, C), dtype=BF16, device=x.device)
    call("ocr_maxpool_fwd", ptr(_dev(x)), ptr(out), Nb, W, H, C, kw, kh, _st())
    return out


def maxpool_bwd(x, dy, kw, kh, relu_mask, out=None):
    Nb, W, H, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    call("ocr_maxpool_bwd", ptr(_dev(x)), ptr(dy), ptr(out), Nb, W, H, C, kw, kh, int(relu_mask), _st())
    return out


def maxpool_bwd_codes(codes, dy, kw, kh, relu_mask, out=None):
    """maxpool_bwd from the routing codes a training forward pass saved (int32 [Nb * W/kw * H/kh, C / 8]: 4 bits per channel, index of the
    window's first maximum | (maximum > 0) << 2) instead of the pool's input; dy is the pooled gradient.  Bit-identical to maxpool_bwd."""
    Nb, Wo, Ho, C = dy.shape
    W, H = Wo * kw, Ho * kh
    assert codes.dtype == torch.int32 and codes.numel() == Nb * Wo * Ho * (C // 8), (codes.dtype, tuple(codes.shape))
    if out is None:
        out = torch.empty((Nb, W, H, C), dtype=BF16, device=dy.device)
    call("ocr_maxpool_bwd_codes", ptr(_dev(codes)), ptr(dy), ptr(out), Nb, W, H, C, kw, kh, int(relu_mask), _st())
    return out


def bn_workspace(M, C, device):
    """Scratch block for bn_train_fwd / bn_train_bwd on [M, C] (ocr_bn_workspace_bytes)."""
    return torch.empty(int(nat.lib().ocr_bn_workspace_bytes(int(M), int(C))), dtype=torch.uint8, device=device)


def bn_train_fwd(x2d, gamma, beta, eps, relu, workspace, out=None, save_mean=None, save_rstd=None, residual=None, partial_rows=0,
                 pooled=None, codes=None):
    """residual (bf16 [M, C]): out = [relu](bf16(bn(x)) + residual) — batch norm, add and relu of a residual block in one apply pass.
    partial_rows > 0: the workspace already holds that many partial statistics rows from the producing convolution (conv3x3_stats);
    pooled (bf16 [M / 2, C]): the 1 x 2 max-pool over row pairs that follows the layer, written by the apply pass.
    codes (int32 [M / 2, C / 8], with pooled): the pool's routing codes are written INSTEAD of the full-resolution output (the returned `out`
    is None) — bn_train_bwd(codes=...) needs nothing else of it."""
    M, C = x2d.shape
    if codes is not None:
        assert pooled is not None and residual is None and out is None
        assert codes.dtype == torch.int32 and tuple(codes.shape) == (M // 2, C // 8), (codes.dtype, tuple(codes.shape))
        if save_mean is None: save_mean = torch.empty(C, dtype=F32, device=x2d.device)
        if save_rstd is None: save_rstd = torch.empty(C, dtype=F32, device=x2d.device)
        call("ocr_bn_train_fwd_codes", ptr(_dev(x2d)), ptr(gamma), ptr(beta), ptr(save_mean), ptr(save_rstd), M, C,
             float(eps), int(relu), ptr(workspace), int(partial_rows), ptr(pooled), ptr(codes), _st())
        return None, save_mean, save_rstd
    if out is None: out = torch.empty_like(x2d)
    if save_mean is None: save_mean = torch.empty(C, dtype=F32, device=x2d.device)
    if save_rstd is None: save_rstd = torch.empty(C, dtype=F32, device=x2d.device)
    if partial_rows or pooled is not None:
        call("ocr_bn_train_fwd2", ptr(_dev(x2d)), ptr(out), ptr(gamma), ptr(beta), ptr(save_mean), ptr(save_rstd), M, C,
             float(eps), int(relu), ptr(workspace), ptr(residual), int(partial_rows), ptr(pooled), _st())
    else:
        call("ocr_bn_train_fwd", ptr(_dev(x2d)), ptr(out), ptr(gamma), ptr(beta), ptr(save_mean), ptr(save_rstd), M, C,
             float(eps), int(relu), ptr(workspace), ptr(residual), _st())
    return out, save_mean, save_rstd


def bn_train_bwd(x2d, y2d, dy2d, gamma, save_mean, save_rstd, dgamma, dbeta, relu, workspace, out=None, pooled_dy=False, partial_rows=0,
                 codes=None):
    """pooled_dy: dy2d is the gradient of the 1 x 2 max-pool behind the layer ([M / 2, C]); the passes route it themselves.
    partial_rows > 0: dy2d is already ReLU-masked and the workspace holds that many partial rows from conv3x3_dgrad_bnbwd.
    codes (with pooled_dy; y2d may be None): what bn_train_fwd(codes=...) saved stands in for y2d."""
    M, C = x2d.shape
    if out is None: out = torch.empty_like(x2d)
    if codes is not None:
        assert pooled_dy and not partial_rows and tuple(dy2d.shape) == (M // 2, C)
        assert codes.dtype == torch.int32 and tuple(codes.shape) == (M // 2, C // 8), (codes.dtype, tuple(codes.shape))
        call("ocr_bn_train_bwd_codes", ptr(_dev(x2d)), ptr(codes), ptr(dy2d), ptr(out), ptr(gamma), ptr(save_mean), ptr(save_rstd),
             ptr(dgamma), ptr(dbeta), M, C, int(relu), ptr(workspace), _st())
        return out
    if pooled_dy or partial_rows:
        assert tuple(dy2d.shape) == ((M // 2, C) if pooled_dy else (M, C))
        call("ocr_bn_train_bwd2", ptr(_dev(x2d)), ptr(y2d), ptr(dy2d), ptr(out), ptr(gamma), ptr(save_mean), ptr(save_rstd),
             ptr(dgamma), ptr(dbeta), M, C, int(relu), ptr(workspace), int(bool(pooled_dy)), int(partial_rows), _st())
    else:
        call("ocr_bn_train_bwd", ptr(_dev(x2d)), ptr(y2d), ptr(dy2d), ptr(out), ptr(gamma), ptr(save_mean), ptr(save_rstd),
             ptr(dgamma), ptr(dbeta), M, C, int(relu), ptr(workspace), _st())
    return out


def bn_train_bwd_codes_col(x2d, codes, col, Nb, W, HC, dy_pooled_out, gamma, save_mean, save_rstd, dgamma, dbeta, relu, workspace, out=None):
    """conv5_col2im(col, dy_pooled_out, Nb, W, HC) + bn_train_bwd(codes=...) with the overlap-add inside the statistics pass: the pooled
    gradient is formed from `col` while the sums are taken and stored to dy_pooled_out for the apply pass.  Bit-identical to the pair."""
    M, C = x2d.shape
    if out is None: out = torch.empty_like(x2d)
    assert codes.dtype == torch.int32 and tuple(codes.shape) == (M // 2, C // 8), (codes.dtype, tuple(codes.shape))
    assert (M // 2) * C == Nb * W * HC and dy_pooled_out.numel() == (M // 2) * C and col.numel() == Nb * (W - 1) * 2 * HC
    call("ocr_bn_train_bwd_codes_col", ptr(_dev(x2d)), ptr(codes), ptr(col), Nb, W, HC, ptr(dy_pooled_out), ptr(out), ptr(gamma),
         ptr(save_mean), ptr(save_rstd), ptr(dgamma), ptr(dbeta), M, C, int(relu), ptr(workspace), _st())
    return out


def conv3x3_stats_rows(Nb, W, H, Cin, Cout, *, bias=True, relu=False):
    """Partial-statistics rows the convolution's epilogue would write for this shape (Nb*W*H / 256), 0 where no kernel with that epilogue
    takes it (host-only query)."""
    flags = (EPI_BIAS if bias else 0) | (EPI_RELU if relu else 0)
    return int(nat.lib().ocr_conv3x3_stats_rows(int(Nb), int(W), int(H), int(Cin), int(Cout), flags))


def conv3x3_bnbwd_rows(Nb, W, H, Cin, Cout):
    """Partial rows conv3x3_dgrad_bnbwd writes for a data gradient of this shape (x = dy [Nb, W, H, Cin] -> dx [.., Cout]); 0: not covered."""
    return int(nat.lib().ocr_conv3x3_bnbwd_rows(int(Nb), int(W), int(H), int(Cin), int(Cout)))


def conv3x3_dgrad_bnbwd(dy, wdgrad, out, mask_y, z, mean, rstd, partials):
    """out = (mask_y > 0) ? conv3x3(dy, wdgrad) : 0 and partials[rows][2][Cout] = per-tile (sum out, sum out * (z - mean) * rstd): the data
    gradient into a batch-norm + ReLU layer together with that layer's batch-norm backward sums."""
    Nb, W, H, Cin = dy.shape
    Cout = wdgrad.shape[0]
    call("ocr_conv3x3_dgrad_bnbwd_bf16", ptr(_dev(dy)), ptr(wdgrad), ptr(out), Nb, W, H, Cin, Cout, ptr(mask_y), ptr(z), ptr(mean), ptr(rstd),
         ptr(partials), _st())
    return out


def conv3x3_stats(x, wpack, out, partials, *, bias=None, relu=False):
    """out = conv3x3(x) (+ bias, optional relu) and partials[rows][2][Cout] (fp32) = per-256-pixel-tile sums / sums of squares of out."""
    Nb, W, H, Cin = x.shape
    Cout = wpack.shape[0]
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_RELU if relu else 0)
    call("ocr_conv3x3_bf16_stats", ptr(_dev(x)), ptr(wpack), ptr(out), Nb, W, H, Cin, Cout, ptr(bias), flags, ptr(partials), _st())
    return out


def bn_infer_fwd(x2d, gamma, beta, mean, var, eps, relu, out):
    M, C = x2d.shape
    call("ocr_bn_infer_fwd", ptr(_dev(x2d)), ptr(out), ptr(gamma), ptr(beta), ptr(mean), ptr(var), M, C, float(eps), int(relu), _st())
    return out


def bn_infer_bwd(x2d, y2d, dy2d, gamma, mean, var, dgamma, dbeta, eps, relu, out):
    M, C = x2d.shape
    call("ocr_bn_infer_bwd", ptr(_dev(x2d)), ptr(y2d), ptr(dy2d), ptr(out), ptr(gamma), ptr(mean), ptr(var), ptr(dgamma), ptr(dbeta),
         M, C, float(eps), int(relu), _st())
    return out


def dropout(src, dst, seed, step_counter, keep_prob):
    """dst = keep ? src / keep_prob : 0 with keep = hash(seed, *step_counter, index) < keep_prob (forward and backward alike)."""
    call("ocr_dropout_bf16", ptr(_dev(src)), ptr(dst), src.numel(), int(seed) & 0xffffffff, ptr(step_counter), float(keep_prob), _st())
    return dst


def avgpool(src, dst, Nb, W, H, C, kw, kh, backward=False):
    call("ocr_avgpool_bf16", ptr(_dev(src)), ptr(dst), Nb, W, H, C, kw, kh, int(backward), _st())
    return dst


def subsample(src, dst, Nb, W, H, C, Wo, Ho, sw, sh, ow, oh, backward=False):
    call("ocr_subsample_bf16", ptr(_dev(src)), ptr(dst), Nb, W, H, C, Wo, Ho, sw, sh, ow, oh, int(backward), _st())
    return dst


def softmax(src_f32, dst_f32):
    C = src_f32.shape[-1]
    call("ocr_softmax_f32", ptr(_dev(src_f32)), ptr(dst_f32), src_f32.numel() // C, C, _st())
    return dst_f32


def colsum(a2d, out, M=None, C=None, lda=None):
    M = a2d.shape[0] if M is None else M
    C = a2d.shape[1] if C is None else C
    lda = a2d.stride(0) if lda is None else lda
    call("ocr_colsum_bf16", ptr(_dev(a2d)), ptr(out), M, C, lda, _st())
    return out


def pack_transpose(w2d, out, lstm_units=0, R=None, Cc=None, ldin=None):
    R = w2d.shape[0] if R is None else R
    Cc = w2d.shape[1] if Cc is None else Cc
    ldin = w2d.stride(0) if ldin is None else ldin
    call("ocr_pack_transpose", ptr(_dev(w2d)), ptr(out), R, Cc, ldin, lstm_units, _st())
    return out


def pack_conv_dgrad(w, out):
    kh, kw, cin, cout = w.shape
    call("ocr_pack_conv_dgrad", ptr(_dev(w)), ptr(out), cin, cout, _st())
    return out


def pack_jobs(table, njobs, total_blocks):
    call("ocr_pack_jobs", ptr(_dev(table)), njobs, total_blocks, _st())


def cast_bf16(src, dst):
    call("ocr_cast_f32_bf16", ptr(_dev(src)), ptr(dst), src.numel(), _st())
    return dst


def u8_to_unit_f32(src_u8, dst_f32):
    """dst = src / 255 (fp32, correctly rounded) — device-side form of groupBatch's `astype(float32) / 255.`"""
    call("ocr_u8_to_unit_f32", ptr(_dev(src_u8)), ptr(dst_f32), src_u8.numel(), _st())
    return dst_f32


def bind_batch(pixels, x, seq_len, seq_len_dst, labels=None, labels_dst=None, labels_len=None, labels_len_dst=None):
    """One launch: device pixels (uint8 -> / 255, or fp32) -> x, plus the int32 vectors into their fixed buffers."""
    is_u8 = pixels.dtype == torch.uint8
    assert pixels.is_contiguous() and pixels.numel() == x.numel() and (is_u8 or pixels.dtype == torch.float32)
    for t in (seq_len, labels, labels_len):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous())
    nl = 0 if labels is None else labels.numel()
    call("ocr_bind_batch", ptr(_dev(pixels)), int(is_u8), ptr(x), pixels.numel(), ptr(_dev(seq_len)), ptr(seq_len_dst), seq_len.numel(),
         ptr(_dev(labels)) if nl else None, ptr(labels_dst) if nl else None, nl,
         ptr(_dev(labels_len)) if labels_len is not None else None, ptr(labels_len_dst) if labels_len is not None else None,
         0 if labels_len is None else labels_len.numel(), _st())


def captcha_synth(params, n_images, words_per_image, atlas, stamp, out, W, stream=None, max_glyphs=None, canvas_cap=1024, width_cap=600,
                  out_h=32):
    """GPU-side captcha synthesis (csrc/captcha_synth.hip): params int32 [n_images * words_per_image (+ more)] device records of
    utils.synth.draw_params -> out uint8 [n_images, W, out_h].  stream: a torch stream (default: the current one)."""
    assert params.dtype == torch.int32 and atlas.dtype == torch.uint8 and stamp.dtype == torch.int32 and out.dtype == torch.uint8
    assert params.numel() >= n_images * words_per_image and out.numel() >= n_images * W * out_h
    if max_glyphs is None:
        max_glyphs = (words_per_image - 92) // 20
    st = _st() if stream is None else stream.cuda_stream
    call("ocr_captcha_synth", ptr(_dev(params)), n_images, words_per_image, max_glyphs, ptr(_dev(atlas)), ptr(_dev(stamp)), stamp.numel() // 2,
         ptr(_dev(out)), W, out_h, canvas_cap, width_cap, st)
    return out


def step_report(costs, scalars, word_addrs, out):
    """out[0..3] (double) = mean cost, scalars[1], scalars[7], bit mask of the error words that read 1 (+ 2^40: this step's update was dropped) — ocr_step_report."""
    nw = 0 if word_addrs is None else word_addrs.numel()
    if scalars is not None and scalars.numel() < optim_scalar_count():
        raise ValueError('step_report: `scalars` must be the whole optimiser block (%d doubles; the report reads entry 72), got %d'
                         % (optim_scalar_count(), scalars.numel()))
    call("ocr_step_report", ptr(_dev(costs)), costs.numel(), ptr(scalars), ptr(word_addrs) if nw else None, nw, ptr(out), _st())
    return out


def cast2d_bf16(src, ldin, dst, ldout, rows, cols):
    call("ocr_cast2d_f32_bf16", ptr(_dev(src)), ldin, ptr(dst), ldout, rows, cols, _st())
    return dst


def tnc_to_ntc_bf16(src_tnc, dst_ntc, scale):
    T, N, C = src_tnc.shape
    call("ocr_tnc_to_ntc_bf16", ptr(_dev(src_tnc)), ptr(dst_ntc), T, N, C, float(scale), _st())
    return dst_ntc


def conv5_col2im(col, dx, Nb, W, HC):
    call("ocr_conv5_col2im", ptr(_dev(col)), ptr(dx), Nb, W, HC, _st())
    return dx


# ----------------------------------------------------------------------------------------------- LSTM
def lstm_fwd_step(xproj, whT, seq_len, hout, gates, cell, Nb, T, U, step, forget_bias=1.0, ndir=2):
    call("ocr_lstm_fwd_step", ptr(_dev(xproj)), ptr(whT), ptr(seq_len), ptr(hout), ptr(gates), ptr(cell), Nb, T, U, step,
         float(forget_bias), ndir, _st())


def lstm_bwd_step(wh, ldw, w_dir_stride, seq_len, dhout, gates, cell, dz, dc_state, Nb, T, U, step, ndir=2):
    call("ocr_lstm_bwd_step", ptr(_dev(wh)), ldw, w_dir_stride, ptr(seq_len), ptr(dhout), ptr(gates), ptr(cell), ptr(dz),
         ptr(dc_state), Nb, T, U, step, ndir, _st())


def set_lstm_ksplit(waves):
    """Waves per workgroup of the persistent LSTM kernels (4: default since round 4; 1: the one-wave kernels).  OCR_LSTM_KSPLIT wins."""
    call("ocr_set_lstm_ksplit", int(waves))


def lstm_seq_test_skew(units, at=-1):
    """Test hook: unit block 0 of every group of the persistent LSTM launches that follow sleeps units x 64 clocks at iteration `at` (< 0: every
    iteration; units 0: off)."""
    call("ocr_lstm_seq_test_skew", int(units), int(at))


def lstm_seq_supported(Nb, U):
    return bool(nat.lib().ocr_lstm_seq_supported(Nb, U))


def lstm_seq_sync_words(Nb, U):
    """int32 words of the persistent kernels' scratch block (group counters | hand-off ring | tail with the error word LAST)."""
    return int(nat.lib().ocr_lstm_seq_sync_words(Nb, U))


LSTM_PREPARED = 1       # OCR_LSTM_PREPARED: every word of `sync` was set to 0xFFFFFFFF earlier on this stream; the call skips its own fill launch


def lstm_fwd_seq(xproj, whT, seq_len, hout, gates, cell, Nb, T, U, sync, forget_bias=1.0, prepared=False):
    call("ocr_lstm_fwd_seq2", ptr(_dev(xproj)), ptr(whT), ptr(seq_len), ptr(hout),
         ptr(gates), ptr(cell), Nb, T, U, float(forget_bias), ptr(sync), LSTM_PREPARED if prepared else 0, _st())


def lstm_fwd_seq_x_supported(Nb, U, D):
    return bool(nat.lib().ocr_lstm_fwd_seq_x_supported(Nb, U, D))


def lstm_fwd_seq_x(x, wxT, bias, whT, seq_len, hout, gates, cell, Nb, T, U, sync, forget_bias=1.0, prepared=False):
    """The forward recurrence with the input projection inside: x bf16 [Nb * T, D]; wxT [2 * 4U, D] / bias [2 * 4U] as gemm_nt takes them."""
    D = x.shape[-1]
    call("ocr_lstm_fwd_seq_x", ptr(_dev(x)), ptr(wxT), ptr(bias), D, ptr(whT), ptr(seq_len), ptr(hout), ptr(gates), ptr(cell),
         Nb, T, U, float(forget_bias), ptr(sync), LSTM_PREPARED if prepared else 0, _st())


def lstm_bwd_seq(wh, ldw, w_dir_stride, seq_len, dhout, gates, cell, dz, Nb, T, U, sync, prepared=False):
    call("ocr_lstm_bwd_seq2", ptr(_dev(wh)), ldw, w_dir_stride, ptr(seq_len),
         ptr(dhout), ptr(gates), ptr(cell), ptr(dz), Nb, T, U, ptr(sync), LSTM_PREPARED if prepared else 0, _st())


def lstm_hprev(hout, seq_len, hprev, Nb, T, U, ndir=2):
    call("ocr_lstm_hprev", ptr(_dev(hout)), ptr(seq_len), ptr(hprev), Nb, T, U, ndir, _st())


def lstm_pack_bias(b_fw, b_bw, out, U, ndir=2):
    call("ocr_lstm_pack_bias", ptr(_dev(b_fw)), ptr(b_bw), ptr(out), U, ndir, _st())


# ----------------------------------------------------------------------------------------------- optimiser
SOLVERS = {"Adam": 0, "Momentum": 1, "RMS": 2}


def optim_scalar_count():
    return int(nat.lib().ocr_optim_scalar_count())


def optim_init(scalars, lr):
    call("ocr_optim_init", ptr(_dev(scalars)), float(lr), _st())


def optim_set_lr(scalars, lr, multiply=False):
    call("ocr_optim_set_lr", ptr(_dev(scalars)), float(lr), int(multiply), _st())


def optim_step(params, grads, state1, state2, reg_range, weight_decay, clip_norm, solver, beta1, beta2, eps, scalars, guard=None, drop_flag=None):
    """reg_range = (begin, end) of the L2-regularised tensors inside the flat buffer.  guard: device int64 tensor of addresses of int words
    that read 1 when a kernel of the step reported invalid results — the update is then dropped on the device; drop_flag: a device float, > 0 =>
    drop (data parallel: the all-reduced guard_flag word, so every rank drops the same step) — ocr_optim_step_guarded2."""
    call("ocr_optim_step_guarded2", ptr(_dev(params)), ptr(grads), ptr(state1), ptr(state2), params.numel(), int(reg_range[0]), int(reg_range[1]),
         float(weight_decay), float(clip_norm), solver, float(beta1), float(beta2), float(eps), ptr(scalars),
         ptr(guard) if guard is not None else None, 0 if guard is None else int(guard.numel()),
         ptr(drop_flag) if drop_flag is not None else None, _st())


def guard_flag(guard, out):
    """out[0] (device float) := 1.0 if any of the int words whose addresses `guard` holds reads 1, else 0.0 (ocr_guard_flag)."""
    call("ocr_guard_flag", ptr(guard) if guard is not None else None, 0 if guard is None else int(guard.numel()), ptr(_dev(out)), _st())
