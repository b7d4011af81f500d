"""tests/errorlocator_numpy.py against the reference's recorded outputs
(tests/golden/errorlocator_fixtures.npz, made by tests/golden/make_golden_errorlocator.py from the
reference's own ErrorLocator and Statistics): the literal do-while and the single pass each equal
every fixture byte for byte, and equal each other on fresh random frames; the statistics
restatement equals the recorded values and their stream-formatted strings."""
import os

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits
from errorlocator_numpy import MODES, default_desired, frozen_mask, locate, locate_literal, statistics
from helpers import LLR_KINDS, llr_kinds

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "errorlocator_fixtures.npz")
_cache = {}


def gold():
    if "z" not in _cache:
        with np.load(GOLD) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def fixture_cases():
    """(case, N, frozen, llr, desired or None, {mode: (u, bits, first, count)}) of every recorded case."""
    z = gold()
    for i, (N, j, F, has) in enumerate(z["meta"].tolist()):
        llr = z[f"c{i}_llr"]
        assert llr.shape == (F, N)
        out = {m: tuple(z[f"c{i}_{m}_{k}"] for k in ("u", "bits", "first", "count")) for m in MODES}
        yield i, N, z[f"code{j}_frozen"].astype(int).tolist(), llr, (z[f"c{i}_desired"] if has else None), out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8),
                                                                                          b.view(np.uint8))


def check(got, want, tag):
    for name, g, w in zip(("u", "bits", "first", "count"), got, want):
        assert same(g, w), (tag, name)


def test_fixture_set_covers_what_it_should():
    counts, Ns, spots, kn1 = [], set(), set(), False
    for i, N, fr, llr, des, out in fixture_cases():
        Ns.add(N)
        kn1 |= len(fr) == 1
        info = np.flatnonzero(~frozen_mask(N, fr))
        first, count = out["correct"][2], out["correct"][3]
        counts += count.tolist()
        assert ((count > 0) == (first >= 0)).all()
        assert (out["reference"][2] == -1).all() and (out["reference"][3] == 0).all()
        assert (out["first"][3] == 0).all() and np.array_equal(out["first"][2], first)
        spots |= {0} if ((first >= 0) & (first // 8 == info[0] // 8)).any() else set()
        spots |= {1} if ((first >= 0) & (first // 8 == info[-1] // 8)).any() else set()
    counts = np.array(counts)
    assert {8, 16, 32, 64, 256, 1024} <= Ns and kn1 and spots == {0, 1}
    assert (counts == 0).any() and (counts == 1).any() and counts.max() >= 64


@pytest.mark.parametrize("form", [locate, locate_literal])
def test_restatements_equal_the_reference(form):
    n = 0
    for i, N, fr, llr, des, out in fixture_cases():
        for mode in MODES:
            check(form(N, fr, llr, des, mode)[:4], out[mode], (i, N, mode))
        n += 1
    assert n >= 30


def test_literal_runs_one_decode_per_correction():
    for i, N, fr, llr, des, out in fixture_cases():
        if N <= 256:
            dec = locate_literal(N, fr, llr, des, "correct")[4]
            assert np.array_equal(dec, out["correct"][3].astype(np.int64) + 1)


def test_the_two_forms_agree_on_fresh_frames():
    rng = np.random.default_rng(77)
    for N, K in ((8, 4), (16, 11), (32, 16), (64, 20), (128, 64)):
        fr = frozen_bits(N, K, 0.0) if N != 16 else sorted(rng.choice(N, N - K, replace=False).tolist())
        llr = np.concatenate([llr_kinds(rng, 3, N, k) for k in LLR_KINDS])
        des = (rng.normal(0, 2, llr.shape)).astype(np.float32)
        des[rng.random(des.shape) < 0.2] = -0.0
        for d in (None, des):
            for mode in MODES:
                a, b = locate(N, fr, llr, d, mode), locate_literal(N, fr, llr, d, mode)
                check(a, b[:4], (N, K, mode, d is None))
        # the defaults, passed explicitly
        check(locate(N, fr, llr, default_desired(N, fr, llr.shape[0])), locate(N, fr, llr, None), (N, "defaults"))


def test_statistics_equal_the_reference():
    from antpolarcodes_amd.errorlocator import fmt
    z = gold()
    n = int(z["stat_count"][0])
    sizes = set()
    for k in range(n):
        vals, out, strs = z[f"stat{k}_values"], z[f"stat{k}_out"], z[f"stat{k}_str"].tolist()
        got = statistics(vals.tolist())
        assert same(np.array(got, np.float32), out), (k, got, out.tolist())
        assert [fmt(v) for v in got[:4]] == strs, (k, strs)
        sizes.add(vals.size)
    assert {0, 1, 2} <= sizes
    assert z["stat1_str"].tolist()[1] in ("-nan", "nan")  # one value: sqrt(0 / 0)
