"""The batches of tests/test_gpu_adaptive_edges.py, built on the CPU: helpers.adaptive_batch
asserts, with the oracle alone, that the first stage fails exactly where each mask says and
that both list outcomes occur among 16 or more failing rows.  Every (code, precision, mask) the
GPU tests decode is built here, so a mask that cannot be reached fails without a GPU."""
import numpy as np
import pytest

import helpers
from helpers import ADAPTIVE_CODES, adaptive_batch, adaptive_case_batch

MI355X_CUS = 256


def _check(b, mask):
    F = len(mask)
    assert np.array_equal(b.mask, mask) and b.frames.shape[0] == F
    assert b.info.shape[0] == F and b.ok.shape == (F,) and b.metrics.shape[0] == F
    assert not b.metrics[~mask].any() and b.ok[~mask].all()
    assert (b.frames.dtype == np.int8) == (b.x8 is not None)


@pytest.mark.parametrize("fixed", [False, True], ids=["float", "char"])
def test_pattern_matrix(oracle, fixed):
    n = 0
    for code, pat, fx, sysm in helpers.adaptive_edge_cases():
        if fx != fixed:
            continue
        _, L, _, b = adaptive_case_batch(oracle, code, pat, fixed, sysm)
        _check(b, helpers.adaptive_pattern(pat, L))
        n += 1
    assert n == len(helpers.ADAPTIVE_PATTERNS) + 4 * (len(ADAPTIVE_CODES) - 1) + 2


@pytest.mark.parametrize("fixed", [False, True], ids=["float", "char"])
def test_no_detector_rows(oracle, fixed):
    """Rows that fail under CRC-8, decoded by a plan without a detector: none reaches the list."""
    N, K, L, _ = ADAPTIVE_CODES["n256_l4"]
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    mask = np.zeros(130, bool)
    b = adaptive_batch(oracle, N, fr, L, 0, mask, fixed=fixed, pool_crc=8)
    _check(b, mask)
    _, ok8 = (oracle.scc_decode if fixed else oracle.sc_decode)(N, fr, b.frames, True, 8)
    assert not ok8.any()


@pytest.mark.parametrize("fixed", [False, True], ids=["float", "char"])
def test_specialised_kernel_batches(oracle, fixed):
    for pat in helpers.SPECIALISED_PATTERNS:
        _, L, crc, b = adaptive_case_batch(oracle, "n1024_l8", pat, fixed, noise=False)
        assert crc == 8  # the catalogue's code
        _check(b, helpers.adaptive_pattern(pat, L))


@pytest.mark.parametrize("fixed", [False, True], ids=["float", "char"])
def test_launch_round_batches(oracle, fixed):
    N, K, L, crc = helpers.ROUNDS_CODE
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    F = helpers.rounds_frames(L, MI355X_CUS)
    assert F == 1031
    for mask in (np.ones(F, bool), np.arange(F) % 3 == 0):
        _check(adaptive_batch(oracle, N, fr, L, crc, mask, fixed=fixed), mask)


@pytest.mark.parametrize("fixed", [False, True], ids=["float", "char"])
def test_sequence_stream_and_chunk_batches(oracle, fixed):
    N, K, L, crc = ADAPTIVE_CODES["n256_l4"]
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    for mask in helpers.sequence_masks(L) + helpers.stream_masks(L) + [helpers.host_chunk_mask(L)]:
        _check(adaptive_batch(oracle, N, fr, L, crc, mask, fixed=fixed), mask)


def test_builder_refuses_a_wrong_mask(oracle):
    """The conditions are asserted, not assumed: rows that do not fail where the mask says stop
    the builder (noise rows under CRC-8 pass the first stage now and then)."""
    N, K, L, _ = ADAPTIVE_CODES["n32_l2"]
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    llr = np.random.default_rng(5).normal(0, 2, (2000, N)).astype(np.float32)
    _, ok = oracle.sc_decode(N, fr, llr, True, 8)
    assert 0 < ok.sum() < len(ok)  # so a batch of them is no "all" mask
    with pytest.raises(AssertionError):
        helpers._assert_first_stage(ok, np.ones(len(ok), bool))
