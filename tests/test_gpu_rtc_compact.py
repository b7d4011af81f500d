"""GPU parity of the specialised list kernel's compacted walk (sclls_kernel.hip, PCG_RTC_COMPACT:
empty positions left out of the table the walk reads, a run of Combines up one node chain done
in registers as one position, a run handed to its parent's G where that is on) against the
interpreter kernel and the oracle, bit for bit in info, ok and the ordered path metrics.

The codes (antpolarcodes_amd/rtc_codes.py compact_codes) hold every kind of walk position, which
tests/test_rtc_compact.py proves on the CPU: N = 32 to 1024, the quarters of N = 1024 recomputed
and stored, list sizes 2, 4, 5 and 8, one non-systematic.  256 frames per code: 128 AWGN-like
and 64 each of the two tie-heavy families of helpers.llr_kinds (integers, {-1, 0, +1}), so exact
ties take the fallback selection."""
import numpy as np
import pytest

from helpers import gpu_plan, llr_kinds
from walk_table import code_id, frozen_of, walk

pytestmark = pytest.mark.gpu

FAMILIES = (("normal", 128), ("ints", 64), ("sparse", 64))
DEFAULT_MODE = 1  # PCG_RTC_COMPACT unset


def _codes():
    from antpolarcodes_amd.rtc_codes import compact_codes
    return compact_codes()


@pytest.mark.parametrize("code", _codes(), ids=code_id)
def test_compacted_walk_matches_interpreter_and_oracle(oracle, code):
    N, L, _, crc, sysm = code
    fr = frozen_of(code)
    rng = np.random.default_rng(9100 + N + L + crc + int(sysm))
    llr = np.concatenate([llr_kinds(rng, n, N, k) for k, n in FAMILIES])
    assert 256 <= llr.shape[0] <= 512
    oi, ook, om, _, _ = oracle.scl_decode(N, L, fr, llr, systematic=sysm, crc=crc, paths=True)
    out = {}
    for kernel in ("rtc", "interp"):
        p = gpu_plan(N, L, fr, kernel=kernel, systematic=sysm, crc=crc)
        assert p.describe()["dev_overrides"] == 0
        if kernel == "rtc":  # (gpu_plan asserted scl_rtc_kernel)
            w = walk(p)
            assert w.mode == DEFAULT_MODE and any(q.kind != 0 for q in w.pos) == (DEFAULT_MODE != 0)
        out[kernel] = p.decode_host(llr, want_metrics=True)
        p.close()
    for kernel, (gi, gok, gm) in out.items():
        lo = 0
        for name, n in FAMILIES:
            sl = slice(lo, lo + n)
            lo += n
            assert np.array_equal(gi[sl], oi[sl]), (kernel, name, "info")
            assert np.array_equal(gok[sl], ook[sl]), (kernel, name, "ok")
            assert np.array_equal(gm[sl].view(np.uint32), om[sl].view(np.uint32)), (kernel, name, "metrics")
    (ri, rok, rm), (ii, iok, im) = out["rtc"], out["interp"]
    assert np.array_equal(ri, ii) and np.array_equal(rok, iok)
    assert np.array_equal(rm.view(np.uint32), im.view(np.uint32))
