"""tests/depthfirst_numpy.py, the checker of the SC-Flip GPU tests, against the reference's own
outputs (tests/golden/depthfirst_fixtures.npz, recorded from Decoding::DepthFirst by
tests/golden/make_golden_depthfirst.py): the decoded codeword words, info bytes, the detector
verdict and the trials run, bit for bit; and the reduced search the kernel runs against the
literal queue of the reference."""
import os

import numpy as np

from depthfirst_numpy import depthfirst_decode, polar_transform_bits, tree_census
from helpers import llr_kinds

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depthfirst_fixtures.npz")
SCAN_GOLD = os.path.join(os.path.dirname(GOLD), "scan_fixtures.npz")


def fixture_cases():
    """(case, N, frozen, limit, crc, systematic, llr, bits, info, ok, trials, depth)"""
    fx = np.load(GOLD, allow_pickle=False)
    for i, (N, j, limit, crc, systematic) in enumerate(fx["meta"]):
        yield (i, int(N), [int(v) for v in fx[f"code{j}_frozen"]], int(limit), int(crc), bool(systematic),
               fx[f"code{j}_llr"], fx[f"c{i}_bits"], fx[f"c{i}_info"], fx[f"c{i}_ok"], fx[f"c{i}_trials"],
               fx[f"c{i}_depth"])


def checker(oracle, crc):
    return (lambda row: oracle.crc(crc, row)) if crc else None


def test_fixture_contents():
    fx = np.load(GOLD, allow_pickle=False)
    meta = fx["meta"]
    assert {8, 16, 32, 64, 256, 1024} <= set(int(v) for v in meta[:, 0])
    assert {1, 2, 3, 4, 8, 32} <= set(int(v) for v in meta[:, 2])
    assert {0, 8, 32} <= set(int(v) for v in meta[:, 3]) and {0, 1} <= set(int(v) for v in meta[:, 4])
    for N, K in ((16, 8), (64, 32), (256, 64), (256, 192), (1024, 512)):
        lim = {int(m[2]) for m in meta if m[0] == N and fx[f"code{m[1]}_frozen"].size == N - K and m[3] == 8}
        assert lim >= {T for T in (1, 2, 3, 4, 8, 32) if K >= T}, (N, K, lim)
    assert fx["ref_cw_per_s"].shape == (2,) and (fx["ref_cw_per_s"] > 0).all()
    assert os.path.getsize(GOLD) <= os.path.getsize(SCAN_GOLD)
    # one case (limit 32) holds all four outcomes of the search
    i = int(fx["mix_case"][0])
    assert meta[i][2] == 32
    ok, tr, dp = fx[f"c{i}_ok"], fx[f"c{i}_trials"], fx[f"c{i}_depth"]
    assert (tr == 1).any() and ((ok == 1) & (tr > 1) & (dp == 0)).any()
    assert ((ok == 1) & (dp == 1)).any() and ((ok == 0) & (tr == 32) & (dp == 1)).any()


def test_reference_known_answer_frame():
    """N = 8, frozen {0, 1, 2, 4}, signal {-5, -6, -4, 1, -4, -5, -7, 2}, no detector: one trial;
    the sign bits of the decoded words are the all-ones codeword."""
    case = next(c for c in fixture_cases() if c[1] == 8)
    _, N, fr, limit, crc, sysm, llr, bits, info, ok, trials, _ = case
    assert fr == [0, 1, 2, 4] and llr.tolist() == [[-5, -6, -4, 1, -4, -5, -7, 2]] and (limit, crc) == (1, 0)
    assert (bits >> 31).tolist() == [[1] * 8] and info.tolist() == [[0xF0]] and ok.tolist() == [1]
    assert trials.tolist() == [1]
    assert tree_census(8, fr) == {"nodes": 15, "leaves": 8, "info_leaves": 4, "frozen_leaves": 4, "short_rater": 7,
                                  "rater": 0, "ops": 1}


def test_restatement_matches_reference(oracle):
    n = 0
    for i, N, fr, limit, crc, sysm, llr, bits, info, ok, trials, depth in fixture_cases():
        st = {}
        w, b, k, t, amb = depthfirst_decode(N, fr, llr, limit, checker(oracle, crc), sysm, stats=st)
        tag = (i, N, limit, crc, sysm)
        assert limit == 1 or not amb.any(), tag  # only unambiguous frames were recorded
        assert np.array_equal(w, bits), (tag, "bits")
        assert np.array_equal(b, info), (tag, "info")
        assert np.array_equal(k, ok), (tag, "ok")
        assert np.array_equal(t, trials), (tag, "trials")
        assert np.array_equal(st["last_depth"], depth), (tag, "depth")
        if limit == 1:
            assert (t == 1).all()
        if crc == 0:  # the dummy detector passes every frame at once
            assert (t == 1).all() and (k == 1).all()
        n += 1
    assert n >= 40


def _check(row):  # a cheap 6-bit detector for the search tests
    return (int(np.bitwise_xor.reduce(row)) * 37 + int(row.sum())) % 64 == 0


def test_reduced_search_equals_the_literal_queue():
    """A few thousand random frames, tie-heavy kinds included, both under the stable rule: the
    same outputs; no decoded configuration deeper than 1; the queue never above T + 1."""
    rng = np.random.default_rng(11)
    frames = deep = 0
    for N, K in ((32, 13), (64, 32), (64, 40)):
        fr = sorted(rng.choice(N, N - K, replace=False).tolist())
        for kind in ("normal", "ints", "sparse", "zeros"):
            for T in (1, 2, 3, 4, 5, 8, 13, 21, 32, K):
                if K < max(T, 2):
                    continue
                llr = llr_kinds(rng, 24, N, kind)
                for sysm in (True, False) if T == 8 else (True,):
                    s1, s2 = {}, {}
                    a = depthfirst_decode(N, fr, llr, T, _check, sysm, stats=s1)
                    b = depthfirst_decode(N, fr, llr, T, _check, sysm, reduced=True, stats=s2)
                    assert all(np.array_equal(x, y) for x, y in zip(a, b)), (N, kind, T)
                    assert (s1["max_queue"], s1["max_depth"]) == (s2["max_queue"], s2["max_depth"])
                    assert np.array_equal(s1["last_depth"], s2["last_depth"])
                    assert s1["max_depth"] <= 1 and s1["max_queue"] <= max(T + 1, 2), (N, kind, T, s1)
                    if kind in ("ints", "sparse") and T > 1:
                        assert a[4].any()  # these kinds do meet ties
                    deep += int(s1["max_depth"] == 1)
                    frames += 2 * llr.shape[0]
    assert frames >= 2000 and deep > 0


def test_queue_bounds_for_every_trial_limit():
    """T = 1 .. 69 on one code with a detector that never passes: decoded depth <= 1 and queue
    <= T + 1 for every limit (what bounds the kernel's search state)."""
    rng = np.random.default_rng(12)
    N, K = 128, 70
    fr = sorted(rng.choice(N, N - K, replace=False).tolist())
    llr = llr_kinds(rng, 3, N, "normal")
    llr[2] *= 8  # every leaf above log(9): the initial queue stops at 2T/3
    for T in range(1, 70):
        st = {}
        out = depthfirst_decode(N, fr, llr, T, lambda row: False, stats=st)
        assert (out[3] == T).all() and (out[2] == 0).all()
        assert st["max_depth"] <= 1 and st["max_queue"] <= T + 1, (T, st)


def test_limit_one_is_plain_sc_and_flips_change_one_decision(oracle):
    rng = np.random.default_rng(13)
    N, fr = 64, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 16, 17, 18, 20, 24, 32, 33, 34, 36, 40, 48]
    llr = llr_kinds(rng, 12, N, "normal")
    isf = np.zeros(N, bool)
    isf[fr] = True
    w, info, ok, t, _ = depthfirst_decode(N, fr, llr, 1, lambda row: False)
    assert (t == 1).all() and (ok == 0).all()
    x = (w >> 31).astype(np.uint8)
    u = polar_transform_bits(x)
    assert not u[:, isf].any()  # a valid codeword of the frozen-bit code
    assert np.array_equal(np.packbits(x[:, ~isf], axis=1), info)
    ns = depthfirst_decode(N, fr, llr, 1, None, systematic=False)
    assert np.array_equal(ns[0], w) and np.array_equal(np.packbits(u[:, ~isf], axis=1), ns[1])
    # limit 2 = the weakest information bit's decision flipped: u differs there first
    w2 = depthfirst_decode(N, fr, llr, 2, lambda row: False)[0]
    u2 = polar_transform_bits((w2 >> 31).astype(np.uint8))
    first = np.argmax(u != u2, axis=1)
    assert (u != u2).any(axis=1).all() and not isf[first].any()
