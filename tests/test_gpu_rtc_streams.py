"""GPU parity of the per-class walk's literal streaming forms (sclls_kernel.hip, PCG_LS_LIT:
literal chunk counts, the last batch pair peeled, per-class batch depths; the shipped kernels
have ls_fgf_lit at depth 4) and of the run-time forms they leave to shared lanes, against the
interpreter kernel and the oracle, bit-exact in info, ok and the ordered path metrics.

The codes (antpolarcodes_amd/rtc_codes.py stream_codes) are the smallest with stages in the
global slab: N = 512 and 1024, list sizes 2, 4 and 8.  On the random frozen sets the first
information bit comes within the first few positions, so the list fills at once and the literal
forms run the stage-6 and stage-7 ops; on the Bhattacharyya sets it comes late, so the first
ops of those stages run with one path whose chunks the lanes share (the run-time forms), the
later ones with a full list.  tests/test_rtc_streams.py checks on the CPU that each code has the
classes meant.  37 frames per LLR family (185 in all): never a multiple of the 64 / LP codewords
of a wave, so the last group is partial; every family of helpers.LLR_KINDS, so exact ties take
the fallback selection."""
import numpy as np
import pytest

from helpers import LLR_KINDS, gpu_plan, llr_kinds

pytestmark = pytest.mark.gpu

FRAMES = 37


def _codes():
    from antpolarcodes_amd.rtc_codes import stream_codes
    return stream_codes()


def _id(c):
    N, L, (kind, arg), crc, sysm = c
    return f"N{N}-L{L}-{kind}{arg if kind != 'set' else len(arg)}-crc{crc}-{'sys' if sysm else 'nonsys'}"


@pytest.mark.parametrize("code", _codes(), ids=_id)
def test_streams_match_interpreter_and_oracle(oracle, code):
    from antpolarcodes_amd.construction import frozen_bits
    N, L, (kind, arg), crc, sysm = code
    fr = list(arg) if kind == "set" else frozen_bits(N, arg, 0.0, kind)
    rng = np.random.default_rng(7100 + N + L)
    llr = np.concatenate([llr_kinds(rng, FRAMES, N, k) for k in LLR_KINDS])
    assert 64 <= llr.shape[0] <= 256
    oi, ook, om, _, _ = oracle.scl_decode(N, L, fr, llr, systematic=sysm, crc=crc, paths=True)
    out = {}
    for kernel in ("rtc", "interp"):
        p = gpu_plan(N, L, fr, kernel=kernel, systematic=sysm, crc=crc)
        assert p.describe()["dev_overrides"] == 0
        out[kernel] = p.decode_host(llr, want_metrics=True)
        p.close()
    for kernel, (gi, gok, gm) in out.items():
        for k, name in enumerate(LLR_KINDS):
            sl = slice(k * FRAMES, (k + 1) * FRAMES)
            assert np.array_equal(gi[sl], oi[sl]), (kernel, name, "info")
            assert np.array_equal(gok[sl], ook[sl]), (kernel, name, "ok")
            assert np.array_equal(gm[sl].view(np.uint32), om[sl].view(np.uint32)), (kernel, name, "metrics")
    (ri, rok, rm), (ii, iok, im) = out["rtc"], out["interp"]
    assert np.array_equal(ri, ii) and np.array_equal(rok, iok)
    assert np.array_equal(rm.view(np.uint32), im.view(np.uint32))
