"""GPU parity of the specialised list kernel's per-class walk (sclls_kernel.hip, PCG_RTC_CLASSES:
one inlined copy of the op per (op code, stage, fused) class, dispatched on a class id) against
the interpreter kernel and the oracle, bit-exact in info, ok and the ordered path metrics.

The codes (antpolarcodes_amd/rtc_codes.py class_codes) are the smallest at which each branch
of the class derivation and of the helpers' stage dispatch first appears: no stage above the
LDS limit (N = 32), stage 3 recomputed (64), slab stages and fused F/G + F (256), two slab
stages (512), and N = 1024 with a leaf at stage top - 2, whose quarters are stored, and without
one, whose quarters are recomputed.  37 frames
per LLR family: never a multiple of the 64 / LP codewords of a wave, so the last group is
partial; every family of helpers.LLR_KINDS, so exact ties take the fallback selection."""
import numpy as np
import pytest

from helpers import LLR_KINDS, gpu_plan, llr_kinds

pytestmark = pytest.mark.gpu

FRAMES = 37


def _codes():
    from antpolarcodes_amd.rtc_codes import class_codes
    return class_codes()


def _id(c):
    N, L, (kind, arg), crc, sysm = c
    return f"N{N}-L{L}-{kind}{arg if kind != 'set' else len(arg)}-crc{crc}-{'sys' if sysm else 'nonsys'}"


@pytest.mark.parametrize("code", _codes(), ids=_id)
def test_class_walk_matches_interpreter_and_oracle(oracle, code):
    from antpolarcodes_amd.construction import frozen_bits
    N, L, (kind, arg), crc, sysm = code
    fr = list(arg) if kind == "set" else frozen_bits(N, arg, 0.0, kind)
    rng = np.random.default_rng(7000 + N + L)
    llr = np.concatenate([llr_kinds(rng, FRAMES, N, k) for k in LLR_KINDS])
    assert llr.shape[0] <= 200
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
