"""A lexicon as a chunked prefix tree (csrc/ctc_trie.hip: ocr_ctc_trie_build, host code), the operand of ops.ctc_score_trie, Engine.score and
Engine.decode(method='lexicon') for dictionaries: every node of the tree runs its CTC recursion once, whatever the number of words below it.

The default chunk size (DESIGN §3 "scoring a dictionary on a prefix tree", measured there): chunks of DEFAULT_CHUNK_NODES = 1024 nodes, the
256-thread kernel form with four nodes a thread; a tree that would make less than MIN_CHUNKS chunks of that size (a chunk is one workgroup
per sample) is cut into chunks of 512 or 256 nodes instead, the sizes at which the forms with two and one node a thread are full; never
fewer than the longest word + 1."""
import ctypes

import numpy as np

from . import _native as nat

DEFAULT_CHUNK_NODES = 1024       # 256 threads x 4 nodes: 16 KiB of LDS a workgroup, eight workgroups a CU
FORM_NODES = (256, 512, 1024)    # what 256 threads hold at 1, 2 and 4 nodes a thread
MIN_CHUNKS = 16                  # 16 chunks x 64 samples = 1024 workgroups on 256 CUs
MAX_LABEL_LEN = 255
LABEL_BITS, PARENT_BITS = 14, 13


def chunk_capacity():
    return int(nat.lib().ocr_ctc_trie_chunk_capacity())


def default_chunk_nodes(total_nodes, deepest):
    """The rule above: total_nodes = nodes of the tree cut into chunks of the capacity, deepest = labels of the longest valid word."""
    share = -(-total_nodes // MIN_CHUNKS)
    return int(max(deepest + 1, [f for f in FORM_NODES if f >= share or f == DEFAULT_CHUNK_NODES][0]))


class LexiconTrie(object):
    """words: label lists (or a pair (dense int32 [K, Lmax], lengths [K]), the ctc_score layout); num_classes = C of the logits it will score;
    blank as the scorer's.  len() and [] give the original label lists back.  The numpy arrays of the builder are kept (nodes,
    chunk_node_start, chunk_word_start, word_node, word_index; node_label / node_parent / node_flag decode the records) and copied to a device
    once per device."""

    def __init__(self, words, num_classes, blank=0, chunk_nodes=None):
        if isinstance(words, tuple) and len(words) == 2 and isinstance(words[0], np.ndarray):
            dense = np.ascontiguousarray(words[0], np.int32)
            lens = np.ascontiguousarray(words[1], np.int32)
            if dense.ndim != 2 or lens.shape != (dense.shape[0],):
                raise ValueError('dense lexicon %s with lengths %s' % (dense.shape, lens.shape))
        else:
            if len(words) == 0:
                raise ValueError('empty lexicon')
            lens = np.array([len(w) for w in words], np.int32)
            dense = np.zeros((len(words), int(lens.max())), np.int32)
            for k, w in enumerate(words):
                dense[k, :len(w)] = w
        if dense.shape[0] == 0:
            raise ValueError('empty lexicon')
        self.dense, self.lengths = dense, lens
        self.num_classes, self.blank = int(num_classes), int(blank)
        self.num_words, self.max_label_len = int(dense.shape[0]), int(dense.shape[1])
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        words_p = p(dense) if dense.size else p(lens)             # (Lmax = 0: no storage, no word of it is read)
        nc, nn = ctypes.c_int(0), ctypes.c_int(0)

        def build(chunk, *arrays):
            nat.call('ocr_ctc_trie_build', words_p, p(lens), self.num_words, self.max_label_len, self.num_classes, self.blank, chunk,
                     ctypes.byref(nc), ctypes.byref(nn), *(arrays or (None,) * 5))

        if chunk_nodes is None:
            inside = np.arange(self.max_label_len)[None, :] < lens[:, None]
            ok = (lens >= 0) & (lens <= min(self.max_label_len, MAX_LABEL_LEN))
            ok &= ~(inside & ((dense < 0) | (dense >= self.num_classes) | (dense == self.blank))).any(axis=1)
            build(chunk_capacity())                               # the size of the tree cut as little as the kernel allows
            chunk_nodes = default_chunk_nodes(nn.value, int(lens[ok].max()) if ok.any() else 0)
        self.chunk_nodes = int(chunk_nodes)
        build(self.chunk_nodes)
        self.num_chunks, self.num_nodes = nc.value, nn.value
        self.nodes = np.empty(self.num_nodes, np.int32)
        self.chunk_node_start = np.empty(self.num_chunks + 1, np.int32)
        self.chunk_word_start = np.empty(self.num_chunks + 1, np.int32)
        self.word_node = np.empty(self.num_words, np.int32)
        self.word_index = np.empty(self.num_words, np.int32)
        build(self.chunk_nodes, p(self.nodes), p(self.chunk_node_start), p(self.chunk_word_start), p(self.word_node), p(self.word_index))
        assert (nc.value, nn.value) == (self.num_chunks, self.num_nodes)
        self._device = {}

    # ---- the node records, decoded
    @property
    def node_label(self):
        return self.nodes & ((1 << LABEL_BITS) - 1)

    @property
    def node_parent(self):
        return (self.nodes >> LABEL_BITS) & ((1 << PARENT_BITS) - 1)

    @property
    def node_flag(self):
        return (self.nodes >> (LABEL_BITS + PARENT_BITS)) & 1

    # ---- a sequence of the original label lists
    def __len__(self):
        return self.num_words

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(self.num_words))]
        k = int(k)
        if k < 0:
            k += self.num_words
        if not 0 <= k < self.num_words:
            raise IndexError(k)
        return self.dense[k, :max(min(int(self.lengths[k]), self.max_label_len), 0)].tolist()

    def device_arrays(self, device):
        """(nodes, chunk_node_start, chunk_word_start, word_node, word_index) as int32 tensors on `device`, copied on the first call."""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._device:
            self._device[device] = tuple(torch.from_numpy(a).to(device) for a in
                                         (self.nodes, self.chunk_node_start, self.chunk_word_start, self.word_node, self.word_index))
        return self._device[device]
