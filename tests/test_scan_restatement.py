"""tests/scan_numpy.py, the checker of the SCAN GPU tests, against the reference's own outputs
(tests/golden/scan_fixtures.npz, recorded from Decoding::Scan by tests/golden/make_golden_scan.py):
soft codeword, extrinsic channel information, info bytes and the CRC-8 verdict, bit for bit
(float32 bit patterns, so that +-0 and inf compare exactly)."""
import os

import numpy as np
import pytest

from scan_numpy import scan_decode

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_fixtures.npz")


def fixture_cases():
    fx = np.load(GOLD, allow_pickle=False)
    for i, (N, j, it, sysm) in enumerate(fx["meta"]):
        yield (int(N), [int(v) for v in fx[f"code{j}_frozen"]], int(it), bool(sysm), fx[f"code{j}_llr"],
               fx[f"c{i}_soft"], fx[f"c{i}_ext"], fx[f"c{i}_info"], fx[f"c{i}_ok"])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_fixture_contents():
    fx = np.load(GOLD, allow_pickle=False)
    meta = fx["meta"]
    assert {8, 16, 64, 128, 256, 1024} <= set(int(v) for v in meta[:, 0])
    assert {1, 2, 4} <= set(int(v) for v in meta[:, 2]) and {0, 1} == set(int(v) for v in meta[:, 3])
    assert fx["ref_cw_per_s"].shape == (2,) and fx["ref_cw_per_s"][0] > 0
    for i in range(len(meta)):
        assert not np.isnan(fx[f"c{i}_soft"]).any() and not np.isnan(fx[f"c{i}_ext"]).any()


def test_reference_known_answer_frame():
    """The reference's own KAT: N = 8, frozen {0, 1, 2, 4}, signal {-5, -6, -4, 1, -4, -5, -7, 2}."""
    want = {1: [-6, -8, -8, -6, -6, -8, -8, -6], 2: [-6, -8, -6, -6, -6, -6, -6, -6]}
    seen = 0
    for N, fr, it, sysm, llr, soft, *_ in fixture_cases():
        if N == 8 and sysm:
            assert fr == [0, 1, 2, 4] and llr.tolist() == [[-5, -6, -4, 1, -4, -5, -7, 2]]
            assert soft.tolist() == [want[it]]
            seen += 1
    assert seen == 2


def test_restatement_matches_reference(oracle):
    n = 0
    for N, fr, it, sysm, llr, soft, ext, info, ok in fixture_cases():
        s, e, b = scan_decode(N, fr, llr, it, sysm)
        assert same_bits(s, soft), (N, it, sysm, "soft")
        assert same_bits(e, ext), (N, it, sysm, "extrinsic")
        assert np.array_equal(b, info), (N, it, sysm, "info")
        assert [int(oracle.crc(8, row)) for row in b] == ok.tolist(), (N, it, sysm, "ok")
        n += 1
    assert n >= 40


@pytest.mark.parametrize("N", [8, 32])
def test_zero_iterations_is_channel_plus_zero(N):
    rng = np.random.default_rng(N)
    llr = rng.normal(0, 2, (3, N)).astype(np.float32)
    llr[:, 0] = -0.0
    s, e, _ = scan_decode(N, [0, 1, 3], llr, 0, True)
    assert same_bits(s, llr + np.float32(0.0)) and same_bits(e, np.zeros_like(llr))
