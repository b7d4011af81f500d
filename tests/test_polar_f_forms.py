"""The identity behind the two-instruction min-sum F (wave.hpp polar_f, PCG_F_FORM 2), on the CPU:

    sign(a ^ b) | min(|a|, |b|)  ==  median(|a|, b, -|a|) ^ sign(a)

with a median in the IEEE total order, which puts -0 below +0.  The clamp of b to [-|a|, +|a|]
is b, +|a| or -|a|; for a = +-0 both bounds are zeros and the total order makes the median the
zero with b's sign.  The three-instruction form (PCG_F_FORM 3: min(|a|, |b|), then the sign) is
the reference's own expression.  Both as 32-bit patterns on the grid and the random pairs of
polar_f_cases.py.

This documents the identity and the +-0 argument.  It says nothing about the hardware's
v_med3_f32: tests/test_gpu_polar_f.py pins that on the device.
"""
import numpy as np

from polar_f_cases import MAG, SIGN, grid, random_pairs, reference_f, special_values


def _key(u):
    """uint32 pattern -> unsigned key monotonic in the IEEE total order (-0 below +0)."""
    u = np.asarray(u, np.uint32)
    return np.where(u & SIGN, ~u, u | SIGN)


def _unkey(k):
    return np.where(k & SIGN, k & MAG, ~k)


def median_form(a, b):
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    keys = np.stack([_key(a & MAG), _key(b), _key((a & MAG) | SIGN)])
    med = _unkey(np.sort(keys, axis=0)[1])
    return med ^ (a & SIGN)


def _inputs():
    ga, gb = grid()
    ra, rb = random_pairs()
    return np.concatenate([ga, ra]), np.concatenate([gb, rb])


def test_total_order_key_round_trips_and_orders_the_zeros():
    v = special_values()
    assert np.array_equal(_unkey(_key(v)), v)
    assert _key(np.uint32(0x80000000)) < _key(np.uint32(0))  # -0 below +0
    f = v.view(np.float32)
    i, j = np.meshgrid(np.arange(v.size), np.arange(v.size), indexing="ij")
    lt = f[i] < f[j]
    assert np.all(_key(v)[i][lt] < _key(v)[j][lt])


def test_inputs_are_what_the_tests_claim():
    v = special_values()
    assert v.size == 36 and np.unique(v).size == 36
    assert not np.isnan(v.view(np.float32)).any()
    ga, gb = grid()
    assert ga.size == 36 * 36
    a, b = random_pairs()
    assert a.size == b.size == 1 << 16
    assert not np.isnan(a.view(np.float32)).any() and not np.isnan(b.view(np.float32)).any()
    q = a.size // 4
    assert np.array_equal(a[:q] & MAG, b[:q] & MAG)
    for sa in (0, 1):
        for sb in (0, 1):  # all four sign combinations of the ties
            assert np.any(((a[:q] >> 31) == sa) & ((b[:q] >> 31) == sb))
    za, zb = (a[q:2 * q] & MAG) == 0, (b[q:2 * q] & MAG) == 0
    assert np.all(za | zb) and za.sum() >= q // 2 and zb.sum() >= q // 2
    assert {int(x) for x in np.unique(a[q:2 * q][za])} == {0, 0x80000000}
    assert {int(x) for x in np.unique(b[q:2 * q][zb])} == {0, 0x80000000}
    a2, b2 = random_pairs()
    assert np.array_equal(a, a2) and np.array_equal(b, b2)  # seeded


def test_reference_f_on_known_values():
    f32 = lambda *x: np.array(x, np.float32).view(np.uint32)  # noqa: E731
    a = f32(3.0, -3.0, 2.0, -2.0, 0.0, -0.0, 0.0, -0.0, np.inf, -np.inf, 1.0)
    b = f32(2.0, 2.0, -3.0, -3.0, 5.0, 5.0, -5.0, -5.0, -np.inf, 7.0, -0.0)
    want = f32(2.0, -2.0, -2.0, 2.0, 0.0, -0.0, -0.0, 0.0, -np.inf, -7.0, -0.0)
    assert np.array_equal(reference_f(a, b), want)


def test_median_form_equals_the_reference():
    a, b = _inputs()
    got, exp = median_form(a, b), reference_f(a, b)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, [(hex(a[i]), hex(b[i]), hex(got[i]), hex(exp[i])) for i in bad[:8]]

