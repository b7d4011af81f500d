"""Inputs and the reference of the min-sum F tests (test_polar_f_forms.py on the CPU,
test_gpu_polar_f.py on the device), all as 32-bit patterns: contract item Q3 makes the sign of
zero observable, and numpy's float comparisons cannot tell -0 from +0.

reference_f restates the reference's F (avx_float.h:55-63): the sign of a ^ b, then the minimum
of the magnitudes.  For non-negative IEEE floats -- zero, denormals, normals, infinity -- the
order of the values is the order of their bit patterns, so the minimum is taken on the patterns
and no host float unit (or its denormal mode) takes part.  No NaN anywhere: NaN LLRs are in no
contract item.
"""
import numpy as np

SIGN = np.uint32(0x80000000)
MAG = np.uint32(0x7FFFFFFF)

_3E9 = int(np.float32(3e9).view(np.uint32))

# magnitudes of the special values; each is taken with both signs (36 values)
SPECIAL_MAGNITUDES = (
    0x00000000,  # zero
    0x00000001, 0x00000002,  # the smallest denormal and its neighbour
    0x007FFFFE, 0x007FFFFF,  # the largest denormal and its neighbour
    0x00800000, 0x00800001,  # the smallest normal and its neighbour
    0x3F000000,  # 0.5
    0x3F7FFFFF, 0x3F800000, 0x3F800001,  # 1 and its two neighbours
    0x40000000,  # 2
    _3E9 - 1, _3E9, _3E9 + 1,  # 3e9 (beyond every int32) and its two neighbours
    0x7F7FFFFE, 0x7F7FFFFF,  # the largest finite and its neighbour
    0x7F800000,  # infinity
)


def special_values():
    m = np.array(SPECIAL_MAGNITUDES, np.uint32)
    return np.concatenate([m, m | SIGN])


def grid():
    """The full cross product of the special values: (a, b) as uint32 patterns."""
    v = special_values()
    a, b = np.meshgrid(v, v, indexing="ij")
    return a.ravel().copy(), b.ravel().copy()


def _random_patterns(rng, n):
    """Half uniform over the non-NaN bit patterns (every exponent, denormals and infinities
    included), half LLR-like normal draws."""
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    nan = (u & MAG) > np.uint32(0x7F800000)
    u[nan] &= np.uint32(0xFF800000)  # a NaN becomes the infinity of its sign
    g = (rng.standard_normal(n) * 4.0).astype(np.float32).view(np.uint32)
    return np.where(rng.integers(0, 2, n).astype(bool), u, g)


def random_pairs(seed=1107, n=1 << 16):
    """n seeded pairs: a quarter with |a| = |b| in all four sign combinations, a quarter from
    {+-0} x random and random x {+-0}, the rest free."""
    rng = np.random.default_rng(seed)
    a, b = _random_patterns(rng, n), _random_patterns(rng, n)
    q = n // 4
    k = np.arange(q)
    # |a| = |b|: the pair's index gives the sign combination
    b[:q] = a[:q] & MAG
    a[:q] = (a[:q] & MAG) | np.where(k & 1, SIGN, np.uint32(0))
    b[:q] |= np.where(k & 2, SIGN, np.uint32(0))
    # a zero of either sign on one side
    z = np.where(k & 1, SIGN, np.uint32(0))
    left = (k & 2) == 0
    a[q:2 * q] = np.where(left, z, a[q:2 * q])
    b[q:2 * q] = np.where(left, b[q:2 * q], z)
    return a, b


def reference_f(a, b):
    """sign(a ^ b) | min(|a|, |b|) on uint32 patterns (no NaN)."""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    return ((a ^ b) & SIGN) | np.minimum(a & MAG, b & MAG)


def describe(a, b, got, exp, limit=12):
    """The first mismatching inputs and outputs, as hex patterns and values."""
    bad = np.flatnonzero(got != exp)
    rows = [f"{bad.size} of {got.size} differ"]
    for i in bad[:limit]:
        rows.append("a %08x (%r)  b %08x (%r)  got %08x  want %08x" % (
            a[i], float(a[i:i + 1].view(np.float32)[0]), b[i], float(b[i:i + 1].view(np.float32)[0]), got[i], exp[i]))
    return "\n".join(rows)
