"""The kernels' min-sum F (wave.hpp polar_f) by itself on the device, below every decoder:
the dev entry pcg_dev_polar_f applies it elementwise, and its output equals the reference's
F -- the sign of a ^ b, the minimum of the magnitudes -- as 32-bit patterns.

Inputs (polar_f_cases.py): the full cross product of 36 special values, both operands (+-0,
the smallest and largest denormal, the smallest normal, +-1, +-3e9, the largest finite, +-inf,
with their neighbours), and 2^16 seeded random pairs, a quarter of them with |a| = |b| in all
four sign combinations and a quarter with a zero of either sign on one side.  No NaN.

What this pins for the median form (PCG_F_FORM 2: v_med3_f32 |a|, b, -|a|, then the sign of a):
that the hardware's median orders -0 below +0 in this operand order (a = +-0 returns the zero
with the sign of a ^ b), that denormals pass unchanged, and that infinities come back as b or
+-|a|.  The form is whichever the library was built with; the default is the one that passes.

Decoder level: every float kernel already has a GPU test that feeds it the "ints" and "zeros"
families through its F stages against the oracle (the list walk: test_gpu_rtc_classes /
_streams / _compact, test_gpu_left_once, test_gpu_scl; Fast-SSC and SC: test_gpu_sc; SCAN,
Fast-SSCAN, SC-Flip, the error locator: test_gpu_scan, _fsscan, _depthfirst, _errorlocator),
so this file adds none."""
import numpy as np
import pytest

from polar_f_cases import describe, grid, random_pairs, reference_f

pytestmark = pytest.mark.gpu


def _run(a, b):
    import torch
    from antpolarcodes_amd import _native
    da = torch.from_numpy(a.view(np.float32).copy()).cuda()
    db = torch.from_numpy(b.view(np.float32).copy()).cuda()
    out, form = _native.dev_polar_f(da, db)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), form


def test_grid_and_random_pairs_bit_exact():
    ga, gb = grid()
    ra, rb = random_pairs()
    a, b = np.concatenate([ga, ra]), np.concatenate([gb, rb])
    got, form = _run(a, b)
    exp = reference_f(a, b)
    assert form in (2, 3, 4)
    assert np.array_equal(got, exp), f"PCG_F_FORM {form}: " + describe(a, b, got, exp)


def test_odd_length_and_own_stream():
    """A length that is no multiple of the block, on a stream of the caller's; and none."""
    import torch
    from antpolarcodes_amd import _native
    ra, rb = random_pairs()
    n = 1000 + 37
    a, b = ra[:n], rb[:n]
    da = torch.from_numpy(a.view(np.float32).copy()).cuda()
    db = torch.from_numpy(b.view(np.float32).copy()).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out, _ = _native.dev_polar_f(da, db)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), reference_f(a, b))
    empty, _ = _native.dev_polar_f(da[:0], db[:0])
    assert empty.numel() == 0
