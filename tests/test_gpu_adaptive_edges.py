"""The adaptive decoders (AdaptiveFloat / AdaptiveChar) at the edges of their failed-frame list.

The second stage decodes fmap[0 .. *fcount), the list compact_failed_kernel builds from the first
stage's ok bytes (capi.cpp decode_adaptive), so its edge is the pattern of failures, not F.
helpers.adaptive_batch builds batches whose first stage fails exactly at a chosen mask (proved
on the CPU by tests/test_adaptive_batches.py); every test here compares info, ok and the path
metrics (float: as bits; 8-bit: the integers; 0 where the first stage passes) with its
expectation: no failure, every frame, one frame at either end, counts around one list wave, a
whole first-stage wave, lists of several launch rounds, one plan over many calls and two
streams, and the host pipeline's chunks."""
import numpy as np
import pytest

import helpers
from helpers import ADAPTIVE_CODES, adaptive_batch, adaptive_case_batch

pytestmark = pytest.mark.gpu

PREC = pytest.mark.parametrize("fixed", [False, True], ids=["float", "char"])


def _plan(N, L, fr, crc, fixed, systematic=True, kernel="interp"):
    """An adaptive plan on the interpreter kernels or on both stages' specialised ones."""
    from antpolarcodes_amd._native import Plan
    if not fixed:
        return helpers.gpu_plan(N, L, fr, kernel, systematic=systematic, crc=crc, adaptive=True)
    p = Plan(N, L, fr, systematic=systematic, crc=crc, device=0, fixed=True, adaptive=True)
    if kernel == "rtc":
        p.specialize()
        assert p.describe()["specialized"] == 1 and p.kernel_name() == "scl_char_rtc_kernel"
    else:
        assert p.describe()["specialized"] == 0 and "rtc" not in p.kernel_name(), p.kernel_name()
    return p


def _same(b, gi, gok, gm, what=""):
    bad = np.nonzero(~(gi == b.info).all(axis=1))[0]
    assert bad.size == 0, f"{what}: info differs in frames {bad[:8]} (failing: {b.mask[bad[:8]]})"
    if gok is not None:
        bad = np.nonzero(gok != b.ok)[0]
        assert bad.size == 0, f"{what}: ok differs in frames {bad[:8]} (failing: {b.mask[bad[:8]]})"
    if gm is not None:
        bad = np.nonzero((gm.view(np.uint32) != b.metrics.view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, f"{what}: metrics differ in frames {bad[:8]} (failing: {b.mask[bad[:8]]})"


def _host(p, b):
    if b.x8 is not None:
        return p.decode_host_i8(b.x8, want_metrics=True)
    return p.decode_host(b.llr, want_metrics=True)


# ------------------------------------------------------------------ failure patterns
@pytest.mark.parametrize("code,pattern,fixed,systematic", helpers.adaptive_edge_cases(),
                         ids=[f"{c}-{p}-{'char' if f else 'float'}{'' if s else '-nonsys'}"
                              for c, p, f, s in helpers.adaptive_edge_cases()])
def test_patterns(oracle, code, pattern, fixed, systematic):
    fr, L, crc, b = adaptive_case_batch(oracle, code, pattern, fixed, systematic)
    p = _plan(ADAPTIVE_CODES[code][0], L, fr, crc, fixed, systematic)
    _same(b, *_host(p, b), what=f"{code} {pattern}")


@PREC
def test_none_no_detector(oracle, fixed):
    """No detector: the first stage's check always passes, whatever the rows (here: rows that
    fail under CRC-8), and the list stage sees an empty list."""
    N, K, L, _ = ADAPTIVE_CODES["n256_l4"]
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    b = adaptive_batch(oracle, N, fr, L, 0, np.zeros(130, bool), fixed=fixed, pool_crc=8)
    assert b.ok.all() and not b.metrics.any()
    _same(b, *_host(_plan(N, L, fr, 0, fixed), b))


@PREC
@pytest.mark.parametrize("pattern", helpers.SPECIALISED_PATTERNS)
def test_patterns_specialised(oracle, pattern, fixed):
    """Both stages on their plan-specialised kernels (the catalogue's (1024, L 8, CRC-8) code)."""
    fr, L, crc, b = adaptive_case_batch(oracle, "n1024_l8", pattern, fixed, noise=False)
    p = _plan(1024, L, fr, crc, fixed, kernel="rtc")
    _same(b, *_host(p, b), what=pattern)


# ------------------------------------------------------------------ lists longer than one launch round
@pytest.mark.parametrize("fixed,variant", [(False, "queue"), (False, "static"), (False, "third"),
                                           (True, "all"), (True, "third")],
                         ids=["float-queue", "float-static", "float-third", "char-all", "char-third"])
def test_launch_rounds(oracle, monkeypatch, fixed, variant):
    """One list wave per CU (PCG_SCL_WPC / PCG_SCLC_WPC = 1) and G (2 cus + 3) + 1 failing frames:
    three rounds for some waves, a partial last group and, for the float kernel, the start
    stagger taken with the list's count -- from the work queue and on the static grid stride;
    "third": the grid still sized by F, a list of about one round."""
    import torch
    monkeypatch.setenv("PCG_SCLC_WPC" if fixed else "PCG_SCL_WPC", "1")
    if variant == "static":
        monkeypatch.setenv("PCG_SCL_QUEUE", "0")
    N, K, L, crc = helpers.ROUNDS_CODE
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    F = helpers.rounds_frames(L, cus)
    mask = np.arange(F) % 3 == 0 if variant == "third" else np.ones(F, bool)
    b = adaptive_batch(oracle, N, fr, L, crc, mask, fixed=fixed)
    _same(b, *_host(_plan(N, L, fr, crc, fixed), b), what=f"F={F}")


# ------------------------------------------------------------------ one plan, many calls
def _device_io(b, L, rows, dev):
    """The batch on the device in tensors of `rows` rows (its F frames first) and prefilled
    outputs: bytes 0xA5, metrics a NaN pattern."""
    import torch
    F = len(b.mask)
    x = torch.zeros((rows, b.frames.shape[1]), dtype=torch.int8 if b.x8 is not None else torch.float32, device=dev)
    x[:F] = torch.from_numpy(b.frames.copy()).to(dev)  # (the batch is shared and read-only)
    info = torch.full((rows, b.info.shape[1]), 0xA5, dtype=torch.uint8, device=dev)
    ok = torch.full((rows,), 0xA5, dtype=torch.uint8, device=dev)
    met = torch.full((rows, L), 0x7FC0A5A5, dtype=torch.int32, device=dev).view(torch.float32)
    return x, info, ok, met


def _device_same(b, io, with_ok, with_met, what):
    """The first F rows are the expectation (or untouched, for an output the call was not given);
    every row beyond them still holds its prefill."""
    F = len(b.mask)
    _, info, ok, met = (t.cpu().numpy() for t in io)
    _same(b, info[:F], ok[:F] if with_ok else None, met[:F] if with_met else None, what)
    assert (info[F:] == 0xA5).all(), f"{what}: info rows beyond F written"
    assert (ok[F if with_ok else 0:] == 0xA5).all(), f"{what}: ok beyond F written"
    assert (met.view(np.uint32)[F if with_met else 0:] == 0x7FC0A5A5).all(), f"{what}: metrics beyond F written"


@PREC
def test_call_sequence(oracle, fixed):
    """Six device-path calls on one plan without a host synchronisation in between: the list
    buffers are reused, keep a longer earlier list (none right after all: outputs the first
    stage's, metrics all zero) and regrow at F = 777; some calls without an ok or a metrics
    buffer (the plan's own ok buffer then feeds the compaction).  Every tensor has rows beyond F
    (at least two), which stay as prefilled."""
    import torch
    N, K, L, crc = ADAPTIVE_CODES["n256_l4"]
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    batches = [adaptive_batch(oracle, N, fr, L, crc, m, fixed=fixed) for m in helpers.sequence_masks(L)]
    use = [(True, True), (False, True), (True, True), (True, False), (True, True), (False, False)]  # (ok, metrics)
    rows = max(len(b.mask) for b in batches) + 2
    dev = torch.device("cuda:0")
    ios = [_device_io(b, L, rows, dev) for b in batches]
    p = _plan(N, L, fr, crc, fixed)
    torch.cuda.synchronize()
    for b, (x, info, ok, met), (wok, wmet) in zip(batches, ios, use):
        F = len(b.mask)
        dec = p.decode_device_i8 if fixed else p.decode_device
        dec(x[:F], info[:F], ok[:F] if wok else None, met[:F] if wmet else None)
    torch.cuda.synchronize()
    for i, (b, io, (wok, wmet)) in enumerate(zip(batches, ios, use)):
        _device_same(b, io, wok, wmet, f"call {i + 1} (F={len(b.mask)})")


@PREC
def test_two_streams_one_plan(oracle, fixed):
    """Two streams alternate calls on one plan -- first on A, all on B, last on A, none on B --
    each into its own outputs, synchronised only at the end: the plan's list buffers are shared,
    so every call is ordered after the one before."""
    import torch
    N, K, L, crc = ADAPTIVE_CODES["n256_l4"]
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    batches = [adaptive_batch(oracle, N, fr, L, crc, m, fixed=fixed) for m in helpers.stream_masks(L)]
    dev = torch.device("cuda:0")
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    ios = [_device_io(b, L, len(b.mask) + 2, dev) for b in batches]
    p = _plan(N, L, fr, crc, fixed)
    torch.cuda.synchronize()
    for i, (b, (x, info, ok, met)) in enumerate(zip(batches, ios)):
        F, s = len(b.mask), (sa, sb)[i % 2]
        for t in (x, info, ok, met):
            t.record_stream(s)
        dec = p.decode_device_i8 if fixed else p.decode_device
        dec(x[:F], info[:F], ok[:F], met[:F], stream=s.cuda_stream)
    torch.cuda.synchronize()
    for i, (b, io) in enumerate(zip(batches, ios)):
        _device_same(b, io, True, True, f"call {i + 1} on stream {'AB'[i % 2]}")


def test_pypolar_mixed(oracle):
    """pypolar's "mixed" decoder: one passing and one failing frame through decode_vector, then a
    g_plus batch through decode_batch."""
    from antpolarcodes_amd import pypolar
    fr, L, crc, b = adaptive_case_batch(oracle, "n256_l4", "g_plus", False)
    dec = pypolar.PolarDecoder(256, L, fr, "mixed")
    dec.setErrorDetection(crc)
    for f in (int(np.nonzero(~b.mask)[0][0]), int(np.nonzero(b.mask)[0][0])):
        assert np.array_equal(dec.decode_vector(b.llr[f]), b.info[f]), f
    assert np.array_equal(dec.decode_batch(b.llr), b.info)


# ------------------------------------------------------------------ host pipeline
@PREC
@pytest.mark.parametrize("mode", ["0", "2"])
def test_host_pipeline_chunks(oracle, monkeypatch, fixed, mode):
    """200 frames in host chunks of 64, 64, 64 and 8, each with its own list: a g_plus spread,
    no failure, every frame, only the last frame -- serial staging and the pinned pipeline;
    8-bit plans from int8 frames and from float frames quantised in the kernels."""
    monkeypatch.setenv("PCG_HOST_CHUNK", "64")
    monkeypatch.setenv("PCG_HOST_PIPE", mode)
    N, K, L, crc = ADAPTIVE_CODES["n256_l4"]
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    b = adaptive_batch(oracle, N, fr, L, crc, helpers.host_chunk_mask(L), fixed=fixed)
    p = _plan(N, L, fr, crc, fixed)
    _same(b, *_host(p, b), what="first call")
    if fixed:
        _same(b, *p.decode_host(b.llr * 10.0, want_metrics=True), what="float frames")
    _same(b, *_host(p, b), what="second call")
