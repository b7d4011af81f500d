"""numpy restatement of the reference's genie-aided SC error locator,
PolarCode::Decoding::ErrorLocator (src/polarcode/decoding/errorlocator.cpp), and of the
`errorlocator` tool's Statistics (src/errorlocator/statistics.cpp).  Test code: the checker of
tests/test_gpu_errorlocator.py, pinned to the reference's own outputs by
tests/test_errorlocator_restatement.py.  The product never imports it.

The tree is createDecoder's: plain SC down to single-bit leaves, every value with the reference's
fp32 expression; the decoded "bits" are 32-bit words (a leaf outputs `replace ? desired : llr`, a
node the word-wise XOR of its children: Combine / CombineBitsShort).  A frozen leaf always
replaces.

Two forms of decode():

  literal      the reference's do-while: a root decode, then findErrors marks the first unreplaced
               information leaf whose sign bit differs from its desired value's; repeated until
               none is left.  corrections + 1 root decodes per frame.
  single pass  one root decode in which each information leaf is compared when it is reached and
               replaced on the spot.  SC is causal (replacing leaf i changes nothing before i), so
               the literal form marks leaves in ascending order and its last decode is this one.
"""
import numpy as np

from scan_numpy import _f

_SIGN = np.uint32(0x80000000)
_INF_WORD = np.uint32(0x7F800000)
f32 = np.float32
MODES = ("reference", "correct", "first")


def frozen_mask(N, frozen):
    isf = np.zeros(N, bool)
    isf[np.asarray(list(frozen), int)] = True
    return isf


def default_desired(N, frozen, F=1):
    """pushBit (:239-246): +inf at a frozen leaf, +0 at an information leaf."""
    d = np.zeros((F, N), f32)
    d[:, frozen_mask(N, frozen)] = np.inf
    return d


def _sc(x, off, leaf):
    """node.decode() with input x (F x n) of the node over leaves [off, off + n): its output words;
    leaf(off, llr words F) -> output words F."""
    n = x.shape[1]
    if n == 1:
        return leaf(off, np.ascontiguousarray(x[:, 0]).view(np.uint32))[:, None]
    h = n // 2
    a, b = np.ascontiguousarray(x[:, :h]), np.ascontiguousarray(x[:, h:])
    left = _sc(_f(a, b), off, leaf)
    g = ((a.view(np.uint32) ^ (left & _SIGN)).view(f32) + b).astype(f32)
    right = _sc(g, off + h, leaf)
    return np.concatenate([left ^ right, right], axis=1)


def _root(llr, leaf):
    with np.errstate(invalid="ignore", over="ignore"):
        return _sc(np.ascontiguousarray(llr, f32), 0, leaf)


def _prep(N, frozen, llr, desired):
    llr = np.ascontiguousarray(llr, f32).reshape(-1, N)
    isf = frozen_mask(N, frozen)
    if desired is None:
        desired = default_desired(N, frozen, llr.shape[0])
    des = np.ascontiguousarray(desired, f32).reshape(-1, N).view(np.uint32)
    assert des.shape == llr.shape
    return llr, isf, des


def locate(N, frozen, llr, desired=None, mode="correct"):
    """The single pass over F frames: (u F x N float32 = getOutput(), bits F x N uint32 =
    getSoftCodeword, first F int32, count F uint32)."""
    assert mode in MODES
    llr, isf, des = _prep(N, frozen, llr, desired)
    F = llr.shape[0]
    u = np.zeros((F, N), np.uint32)
    first, count = np.full(F, -1, np.int32), np.zeros(F, np.uint32)

    def leaf(i, v):
        d = des[:, i]
        if isf[i]:
            out = d
        else:
            miss = (((d ^ v) & _SIGN) != 0) & (mode != "reference")
            first[miss & (first < 0)] = i
            if mode == "correct":
                count[miss] += 1
                out = np.where(miss, d, v)
            else:
                out = v
        u[:, i] = out
        return out

    bits = _root(llr, leaf)
    return u.view(f32), bits, first, count


def locate_literal(N, frozen, llr, desired=None, mode="correct"):
    """The reference's statements, frame by frame: ErrorLocator::decode as the reference decoder
    or with prepare / do-while / findErrors, and decodeFindFirstError.  Same outputs as locate,
    and the root decodes each frame took."""
    assert mode in MODES
    llr, isf, des = _prep(N, frozen, llr, desired)
    F = llr.shape[0]
    info = np.flatnonzero(~isf)
    u, bits = np.zeros((F, N), np.uint32), np.zeros((F, N), np.uint32)
    first, count, decodes = np.full(F, -1, np.int32), np.zeros(F, np.uint32), np.zeros(F, np.int64)
    for f in range(F):
        replace = isf.copy()  # prepare(): the information leaves' flags cleared
        value = np.zeros(N, np.uint32)

        def leaf(i, v):
            value[i] = des[f, i] if replace[i] else v[0]
            return value[i:i + 1].copy()

        while True:
            bits[f] = _root(llr[f:f + 1], leaf)[0]
            decodes[f] += 1
            if mode == "reference":
                break
            hit = -1
            for i in info:  # findErrors / findFirstError
                if ((des[f, i] ^ value[i]) & _SIGN) and not replace[i]:
                    hit = int(i)
                    break
            if mode == "first":
                first[f] = hit
                break
            if hit < 0:
                break
            replace[hit] = True
            if count[f] == 0:
                first[f] = hit
            count[f] += 1
        u[f] = value
    return u.view(f32), bits, first, count, decodes


def statistics(values):
    """Statistics::evaluate (statistics.cpp:24-61) in float32 and in insertion order:
    (mean, dev, min, max, sum).  Empty: all zero (`return { 0 }`).  The scan is the reference's
    `if (x < min) ... else if (x > max)`; dev divides by size - 1, so one value gives sqrt(0 / 0)."""
    c = [f32(v) for v in values]
    if not c:
        z = f32(0)
        return z, z, z, z, z
    size = len(c)
    mn = mx = 0
    s = f32(0)
    for i in range(size):
        s = f32(s + c[i])
        if c[i] < c[mn]:
            mn = i
        elif c[i] > c[mx]:
            mx = i
    mean = f32(s / f32(size))
    total = s
    s = f32(0)
    for i in range(size):
        t = f32(c[i] - mean)
        s = f32(s + f32(t * t))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = f32(s) / f32(size - 1)  # float / unsigned: the unsigned converts to float
        if size == 1:  # 0.0f / 0.0f: x86's default NaN has its sign bit set, and sqrt keeps it
            q = np.array([0xFFC00000], np.uint32).view(f32)[0]
        dev = f32(np.sqrt(f32(q)))
    return mean, dev, c[mn], c[mx], total
