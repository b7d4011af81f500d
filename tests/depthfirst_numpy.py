"""numpy restatement of the reference's SC-Flip decoder, PolarCode::Decoding::DepthFirst
(src/polarcode/decoding/depth_first.cpp).  Test code: the checker of tests/test_gpu_depthfirst.py,
pinned to the reference's own outputs by tests/test_depthfirst_restatement.py.  The product never
imports it.

The tree is createDecoder's: plain SC down to single bits (the Repetition / SPC branches are
commented out in the reference), every value with the reference's fp32 expression; the decoded
"bits" are 32-bit words (an information leaf outputs its LLR, negated when its option is 1, a
frozen leaf +inf, a node the word-wise XOR of its children: Combine / CombineBitsShort).  A pass
runs over all frames that still decode; the search (Manager::decode / decodeNext) runs per frame.

Two forms of the search:

  literal  the reference's queue of configurations (depth, node list, options), its rotate, its
           sorts and its size tests, statement for statement.
  reduced  what the kernel keeps: the first T leaves of the first pass's order, one extra leaf
           per popped depth-0 configuration (the least reliable leaf outside its prefix, from that
           configuration's own decode), and the queue-size counter that decides whether children
           are pushed.  Children of depth-1 configurations only count: they are never decoded
           within T trials (tests/test_depthfirst_restatement.py).

Ties.  Where two leaves have equal reliability, std::sort's order is a property of libstdc++, not
of the decoder.  Both forms here send ties to the lower leaf index (a sort by (reliability, leaf
index); strict < in the min-selection).  `ambiguous` is set for a frame when a selection that can
reach a decode (the first pass's positions in use, a popped depth-0 configuration's extra leaf)
had an equal neighbour at the position it used; only frames without that flag are comparable
with the reference.
"""
import math
from collections import deque

import numpy as np

from scan_numpy import _f

_SIGN = np.uint32(0x80000000)
_INF_WORD = np.uint32(0x7F800000)
LOG9 = math.log(9.0)  # the reference compares a float promoted to double with log(9)
f32 = np.float32


def tree_census(N, frozen):
    """createDecoder's tree: all nodes (RateR / ShortRateR and the single-bit leaves), and what
    the kernel's plan derives from it: one op per size-8 subtree, three (F, G, combine) per larger
    node."""
    isf = np.zeros(N, bool)
    isf[np.asarray(list(frozen), int)] = True
    return {"nodes": 2 * N - 1, "leaves": N, "info_leaves": int((~isf).sum()), "frozen_leaves": int(isf.sum()),
            "short_rater": sum(N >> k for k in range(1, 4)), "rater": max(N // 8 - 1, 0),
            "ops": N // 8 + 3 * (N // 8 - 1)}


def _sc(x, isf, rank, off, flip, rel):
    """node.decode() with input x (F x n) of the node over leaves [off, off + n): its output words."""
    n = x.shape[1]
    if n == 1:
        if isf[off]:  # RateZeroDecoder
            return np.full((x.shape[0], 1), _INF_WORD, np.uint32)
        r = rank[off]  # RateOneDecoder of block length 1
        rel[:, r] = np.abs(x[:, 0])
        return np.ascontiguousarray(x).view(np.uint32) ^ (flip[:, r:r + 1].astype(np.uint32) << np.uint32(31))
    h = n // 2
    a, b = np.ascontiguousarray(x[:, :h]), np.ascontiguousarray(x[:, h:])
    left = _sc(_f(a, b), isf, rank, off, flip, rel)
    g = ((a.view(np.uint32) ^ (left & _SIGN)).view(f32) + b).astype(f32)
    right = _sc(g, isf, rank, off + h, flip, rel)
    return np.concatenate([left ^ right, right], axis=1)


def sc_pass(llr, isf, flip):
    """One root decode of F frames: (words F x N uint32, reliabilities F x K float32).  flip
    (F x K bool) marks the information leaves whose option is 1."""
    rank = np.cumsum(~isf) - 1
    rel = np.zeros((llr.shape[0], int((~isf).sum())), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        words = _sc(np.ascontiguousarray(llr, f32), isf, rank, 0, flip, rel)
    return words, rel


def _tie(rel, order, pos):
    v = rel[order[pos]]
    return (pos > 0 and rel[order[pos - 1]] == v) or (pos + 1 < len(order) and rel[order[pos + 1]] == v)


class LiteralSearch:
    """Manager::decode / decodeNext with the queue of configurations as the reference keeps it."""

    def __init__(self, T):
        self.T, self.queue, self.first = T, deque(), True
        self.ambiguous, self.max_queue, self.max_depth = False, 0, 0

    def start(self, rel):  # Manager::decode after the first root decode
        T = self.T
        order = sorted(range(len(rel)), key=lambda i: (rel[i], i))
        n = 0
        while True:
            lst = order if n == 0 else [order[n]] + order[:n] + order[n + 1:]  # std::rotate
            for opt in ((0, 1) if n == 0 else (1,)):
                self.queue.append((0, lst, [opt]))
            self.ambiguous |= _tie(rel, order, n)
            n += 1
            if not ((n < T * 2 // 3 or float(rel[order[n]]) < LOG9) and len(self.queue) < T):
                break
        self.max_queue = len(self.queue)

    def next(self, rel):  # Manager::decodeNext; rel: the reliabilities of the last decode
        depth, lst, opts = self.queue.popleft()
        if len(self.queue) < self.T:
            if not self.first:
                lst = lst[:depth + 1] + sorted(lst[depth + 1:], key=lambda i: (rel[i], i))
            if depth == 0:
                self.ambiguous |= depth + 2 < len(lst) and rel[lst[depth + 1]] == rel[lst[depth + 2]]
                if self.first:
                    self.ambiguous |= _tie(rel, lst, 1)
            for opt in (0, 1):
                self.queue.append((depth + 1, lst, opts + [opt]))
        self.first = False
        self.max_queue = max(self.max_queue, len(self.queue))
        depth, lst, opts = self.queue[0]
        self.max_depth = max(self.max_depth, depth)
        return [lst[i] for i in range(depth + 1) if opts[i]]


class ReducedSearch:
    """The kernel's search state: entries (prefix leaves, options, depth) of the configurations in
    queue order, as far as T trials can reach them, and the queue-size counter."""

    def __init__(self, T):
        self.T, self.entries, self.count, self.qsize, self.popped = T, [], 0, 0, 0
        self.ambiguous, self.max_queue, self.max_depth = False, 0, 0

    def _push(self, e):
        if self.count < self.T:
            self.entries.append(e)
        self.count += 1

    @staticmethod
    def _select(rel, after):
        """The next leaf in (reliability, index) order after `after` = (value, index)."""
        idx = np.arange(rel.size)
        m = (rel > after[0]) | ((rel == after[0]) & (idx > after[1]))
        i = int(np.argmin(np.where(m, rel, np.inf)))
        return i, (rel[i], i)

    def start(self, rel):
        T = self.T
        order, after = [], (f32(-np.inf), -1)
        for _ in range(min(T + 1, rel.size)):  # the first T leaves (one more: the tie test's neighbour)
            i, after = self._select(rel, after)
            order.append(i)
        self.ord1, self.amb1 = order[1], _tie(rel, order, 1)
        n = 0
        while True:
            for opt in ((0, 1) if n == 0 else (1,)):
                self._push(((order[n],), (opt,)))
            self.ambiguous |= _tie(rel, order, n)
            n += 1
            if not ((n < T * 2 // 3 or float(rel[order[n]]) < LOG9) and self.count < T):
                break
        self.qsize = self.max_queue = self.count

    def next(self, rel):
        leaves, opts = self.entries[self.popped]
        self.qsize -= 1
        if self.qsize < self.T:
            if len(leaves) == 1:
                if self.popped == 0:
                    w = self.ord1
                    self.ambiguous |= self.amb1
                else:
                    r = np.array(rel, f32)
                    r[leaves[0]] = np.inf
                    w = int(np.argmin(r))
                    self.ambiguous |= bool((r == r[w]).sum() > 1)
                for opt in (0, 1):
                    self._push((leaves + (w,), opts + (opt,)))
            else:  # children of a depth-1 configuration: counted, never decoded
                self._push(None)
                self._push(None)
            self.qsize += 2
        self.max_queue = max(self.max_queue, self.qsize)
        self.popped += 1
        leaves, opts = self.entries[self.popped]
        self.max_depth = max(self.max_depth, len(leaves) - 1)
        return [v for v, o in zip(leaves, opts) if o]


def polar_transform_bits(bits):
    """x -> x G over GF(2) along the last axis (natural order; G is its own inverse)."""
    x = np.array(bits, np.uint8)
    N, B = x.shape[-1], 1
    while B < N:
        v = x.reshape(x.shape[:-1] + (N // (2 * B), 2, B))
        v[..., 0, :] ^= v[..., 1, :]
        B *= 2
    return x


def info_bytes(words, isf, systematic):
    bits = (words >> np.uint32(31)).astype(np.uint8)
    if not systematic:  # setFloatCodeword, encode() (non-systematic), getInformation
        bits = polar_transform_bits(bits)
    return np.packbits(bits[:, ~isf], axis=1)


def depthfirst_decode(N, frozen, llr, T, check=None, systematic=True, reduced=False, stats=None):
    """DepthFirst::decode over F frames: returns (codeword words F x N uint32, info bytes
    F x ceil(K/8), ok F, trials run F, ambiguous F).  check(info_row) -> bool is the detector
    (None: the dummy detector, which passes every frame).  stats (a dict) receives the largest
    queue size and decoded depth, and per frame the depth of the last decoded configuration."""
    llr = np.ascontiguousarray(llr, f32).reshape(-1, N)
    F = llr.shape[0]
    isf = np.zeros(N, bool)
    isf[np.asarray(list(frozen), int)] = True
    K = int((~isf).sum())
    assert 1 <= T <= 255 and K >= max(T, 2)
    words = np.zeros((F, N), np.uint32)
    info = np.zeros((F, (K + 7) // 8), np.uint8)
    ok, ntr, amb = np.zeros(F, np.uint8), np.zeros(F, np.uint8), np.zeros(F, bool)
    last_depth, depth_now = np.zeros(F, np.int8), np.zeros(F, np.int8)
    search = [(ReducedSearch if reduced else LiteralSearch)(T) for _ in range(F)]
    act = np.arange(F)
    flip = np.zeros((F, K), bool)
    for run in range(1, T + 1):
        w, rel = sc_pass(llr[act], isf, flip[act])
        b = info_bytes(w, isf, systematic)
        good = np.array([True if check is None else bool(check(row)) for row in b], bool)
        words[act], info[act], ok[act], ntr[act] = w, b, good, run
        last_depth[act] = depth_now[act]
        keep = ~good
        if run == T or not keep.any():
            break
        rel, act = rel[keep], act[keep]
        for k, fidx in enumerate(act):
            s = search[fidx]
            if run == 1:
                s.start(rel[k])
            fl = s.next(rel[k])
            flip[fidx] = False
            flip[fidx, fl] = True
            depth_now[fidx] = (len(s.entries[s.popped][0]) - 1) if reduced else s.queue[0][0]
    for fidx in range(F):
        amb[fidx] = search[fidx].ambiguous
    if stats is not None:
        stats["max_queue"] = max([s.max_queue for s in search] + [0])
        stats["max_depth"] = max([s.max_depth for s in search] + [0])
        stats["last_depth"] = last_depth
    return words, info, ok, ntr, amb
