"""numpy restatement of the reference's Fast-SSCAN decoder
(src/polarcode/decoding/fastsscan_float.cpp), vectorised over frames.  Test code: the checker of
tests/test_gpu_fsscan.py, pinned to the reference's own outputs by
tests/test_fsscan_restatement.py.  The product never imports it.

It follows the reference's node classes (createDecoder's order of tests, RateRNode::decode,
RepetitionNode::decode, TwoBitNode::decode, reset()), not the kernel's schedule: every value has
the reference's fp32 expression.  Two switches:

  carry   True reproduces ONE reused reference instance: TwoBitNode::reset() is empty, so a
          TwoBit node that is a right child still holds its previous frame's message where its
          parent first reads it (frame 0 starts from +0).  False (the product's behaviour)
          starts every frame from +0 there, which is a freshly constructed reference decoder.
  forced  run exactly `trials` passes and check only after the last (decodeAgain() after t
          passes = t + 1 forced passes).
"""
import numpy as np

from scan_numpy import _f

ZERO, ONE, TWO, REP, RATER = "zero", "one", "two", "rep", "rater"
f32 = np.float32


class Node:
    def __init__(self, isf, right_child=False):
        n, nf = isf.size, int(isf.sum())
        self.n, self.right_child = n, right_child
        self.left = self.right = None
        if nf == n:  # createDecoder (fastsscan_float.cpp:238-265), in its order
            self.kind = ZERO
        elif nf == 0:
            self.kind = ONE
        elif n == 2:
            self.kind = TWO
        elif nf == n - 1:
            self.kind = REP
        else:
            self.kind = RATER
            self.left, self.right = Node(isf[:n // 2]), Node(isf[n // 2:], True)

    def walk(self):
        yield self
        if self.kind == RATER:
            yield from self.left.walk()
            yield from self.right.walk()


def tree(N, frozen):
    isf = np.zeros(N, bool)
    isf[np.asarray(list(frozen), int)] = True
    return Node(isf), isf


def fsscan_census(N, frozen):
    """Node kinds of the tree, and what the kernel's plan derives from them: `ops` (one per RateR
    phase whose child is not a constant node, one per Repetition and TwoBit node, one for a
    constant root), `right_floats` (messages of the non-constant right children, each padded to a
    multiple of 4) and `right_twobit` (TwoBit nodes that are right children)."""
    root, _ = tree(N, frozen)
    c = {ZERO: 0, ONE: 0, TWO: 0, REP: 0, RATER: 0, "ops": 0, "right_floats": 0, "right_twobit": 0}
    for nd in root.walk():
        c[nd.kind] += 1
        if nd.kind in (TWO, REP):
            c["ops"] += 1
        if nd.kind == TWO and nd.right_child:
            c["right_twobit"] += 1
        if nd.kind == RATER:
            c["ops"] += 1 + (nd.left.kind not in (ZERO, ONE)) + (nd.right.kind not in (ZERO, ONE))
            if nd.right.kind not in (ZERO, ONE):
                c["right_floats"] += (nd.right.n + 3) // 4 * 4
    if root.kind in (ZERO, ONE):
        c["ops"] += 1
    c["nodes"] = c[ZERO] + c[ONE] + c[TWO] + c[REP] + c[RATER]
    return c


def _const(nd, F):
    return np.full((F, nd.n), np.inf if nd.kind == ZERO else 0.0, f32)


def _run(nd, x, st):
    """nd.decode() with input x (F x n): the node's message.  st: messages of the right children
    as the previous pass (or reset()) left them, by node."""
    F = x.shape[0]
    if nd.kind in (ZERO, ONE):  # never visited: the message reset() wrote
        return _const(nd, F)
    if nd.kind == TWO:
        return np.ascontiguousarray(x[:, ::-1])
    if nd.kind == REP:
        if nd.n < 8:
            s = np.zeros(F, f32)
            for i in range(nd.n):
                s = s + x[:, i]
        else:
            p = np.zeros((F, 8), f32)
            for k in range(nd.n // 8):
                p = p + x[:, 8 * k:8 * k + 8]
            s = p[:, 0] + p[:, 1]
            for j in range(2, 8):
                s = s + p[:, j]
        return (s[:, None] - x).astype(f32)
    h = nd.n // 2
    a, b = np.ascontiguousarray(x[:, :h]), np.ascontiguousarray(x[:, h:])
    er = st[nd.right]
    el = _run(nd.left, _f(er + b, a), st)
    er = _run(nd.right, _f(el, a) + b, st)
    st[nd.right] = er
    return np.concatenate([_f(el, er + b), er + _f(el, a)], axis=1)


def _reset(root, F, prev=None):
    """reset(): +0 for One, Repetition and RateR, +inf for Zero; a TwoBit node keeps `prev`'s
    message (carry) or starts from +0."""
    st = {}
    for nd in root.walk():
        if nd.kind == RATER:
            r = nd.right
            if r.kind == TWO and prev is not None:
                st[r] = prev[r]
            else:
                st[r] = _const(r, F) if r.kind == ZERO else np.zeros((F, r.n), f32)
    return st


def _decode(root, isf, llr, trials, check, forced, prev):
    F, N = llr.shape
    st = _reset(root, F, prev)
    soft = np.zeros((F, N), f32)
    info = np.zeros((F, (N - int(isf.sum()) + 7) // 8), np.uint8)
    ok = np.zeros(F, np.uint8)
    ntr = np.zeros(F, np.uint8)
    active = np.ones(F, bool)
    for t in range(1, trials + 1):
        s = llr + _run(root, llr, st)  # calculateOutput
        bits = np.packbits((np.ascontiguousarray(s).view(np.uint32) >> 31).astype(np.uint8)[:, ~isf], axis=1)
        good = np.array([True if check is None else bool(check(row)) for row in bits], bool)
        soft[active], info[active], ok[active], ntr[active] = s[active], bits[active], good[active], t
        if not forced:
            active &= ~good
            if not active.any():
                break
    return soft, info, ok, ntr, st


def fsscan_decode(N, frozen, llr, trials, check=None, carry=False, forced=False):
    """FastSscanFloat::decode over F frames: returns (soft codeword F x N, info bytes
    F x ceil(K/8), ok F, passes run F).  check(info_row) -> bool is the detector (None: the
    dummy detector, which passes every frame)."""
    llr = np.ascontiguousarray(llr, f32).reshape(-1, N)
    root, isf = tree(N, frozen)
    if not carry:
        return _decode(root, isf, llr, trials, check, forced, None)[:4]
    outs, prev = [], None
    for f in range(llr.shape[0]):  # one reused decoder: frame by frame
        *o, prev = _decode(root, isf, llr[f:f + 1], trials, check, forced, prev)
        outs.append(o)
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(4))
