"""The root's left child staged once per codeword (sclls_kernel.hip, PCG_STG_LEFT_ONCE), on the
CPU (no GPU): the scratch slab of a host-only plan holds the wave's images where the quarters /
eighths are recomputed, the switch is a plan property, and the codes of
tests/test_gpu_left_once.py have the path counts at the left half's staged ops that the test is
about."""
import ctypes

import pytest

OP_S_R1, OP_S_REP, OP_S_SPC, OP_S_ST8 = 41, 42, 43, 44


def _frozen(c):
    from antpolarcodes_amd.construction import frozen_bits
    N, L, (kind, arg), crc, sysm = c
    return [int(v) for v in (arg if kind == "set" else frozen_bits(N, arg, 0.0, kind))]


def _plan(c):
    from antpolarcodes_amd._native import Plan
    N, L, spec, crc, sysm = c
    return Plan(N, L, _frozen(c), systematic=sysm, crc=crc, device=-1)


# (N, L): bytes of one wave's slab without the images -- the alpha stages [Sl, top - V) of 64
# lanes, the 4 KB tie list and, with D buffers (L = 32), the global D stages -- and V
_SLAB = {
    (512, 8): (4 * (64 * (2 ** 8 - 2 ** 6) + 1024), 1),     # quarters stored: no image
    (512, 2): (4 * (64 * (2 ** 8 - 2 ** 6) + 1024), 1),
    (1024, 8): (4 * (64 * (2 ** 8 - 2 ** 6) + 1024), 2),
    (1024, 4): (4 * (64 * (2 ** 8 - 2 ** 6) + 1024), 2),
    (1024, 2): (4 * (64 * (2 ** 8 - 2 ** 6) + 1024), 2),
    (4096, 32): (4 * (64 * (2 ** 9 - 2 ** 6) + 1024 + 64 * (2 ** 8 - 2 ** 5)), 3),
}


@pytest.mark.parametrize("N,L", sorted(_SLAB))
def test_scratch_holds_one_image_per_codeword(N, L):
    """G x N/2 floats after the slab's other regions where stage top-2 is recomputed (N >= 1024:
    68 KB per wave for config 3, 52 KB before), nothing at N = 512, whose quarters are stored."""
    from antpolarcodes_amd.construction import frozen_bits
    from antpolarcodes_amd._native import Plan
    p = Plan(N, L, frozen_bits(N, N // 2, 0.0), systematic=True, crc=8, device=-1)
    d = p.describe()
    base, virt = _SLAB[(N, L)]
    assert d["recomputed_stages"] == virt
    G = 64 // d["lanes_per_codeword"]
    image = 4 * G * (N // 2) if virt >= 2 else 0
    assert d["scratch_bytes"] == base + image, (d["scratch_bytes"], base, image)
    assert d["dev_overrides"] == 0
    p.close()


def test_scratch_of_2048_waves_stays_in_the_last_level_cache():
    from antpolarcodes_amd.construction import frozen_bits
    from antpolarcodes_amd._native import Plan
    p = Plan(1024, 8, frozen_bits(1024, 512, 0.0), systematic=True, crc=8, device=-1)
    assert p.describe()["scratch_bytes"] == 68 * 1024
    assert 2048 * p.describe()["scratch_bytes"] <= (256 << 20) * 6 // 10
    p.close()


def test_switch_is_a_plan_property(monkeypatch):
    """PCG_SCL_LEFT_ONCE=0/1 is read at plan creation, changes the specialised kernel's source
    (its fuse literal), hence its cache name, and is reported as a developer switch; 1 is the
    default spelled out."""
    from antpolarcodes_amd._native import Plan, lib
    from antpolarcodes_amd.construction import frozen_bits
    names = {}
    for v in (None, "0", "1"):
        if v is None:
            monkeypatch.delenv("PCG_SCL_LEFT_ONCE", raising=False)
        else:
            monkeypatch.setenv("PCG_SCL_LEFT_ONCE", v)
        p = Plan(1024, 8, frozen_bits(1024, 512, 0.0), systematic=True, crc=8, device=-1)
        b = ctypes.create_string_buffer(256)
        assert lib().pcg_dev_rtc_cache_name(p._h, b, 256) == 0
        names[v] = b.value
        assert p.describe()["dev_overrides"] == (0 if v is None else 0x2)
        assert p.describe()["scratch_bytes"] == 68 * 1024  # (the layout does not depend on it)
        p.close()
    assert names[None] == names["1"] != names["0"]


def _branching_leaves(c, lo, hi):
    """Leaves of the plan's schedule inside [lo, hi) that hold an information bit: each at
    least doubles the path count until it is L."""
    from antpolarcodes_amd._native import lib
    p = _plan(c)
    ops = (ctypes.c_uint32 * 16384)()
    nops = lib().pcg_dev_plan_ops(p._h, ops, 16384)
    assert 0 < nops <= 16384
    virt = p.describe()["recomputed_stages"]
    p.close()
    fr = set(_frozen(c))
    n, k = 0, 0
    while k < nops:
        w = ops[k]
        opc, stage, off = w & 0xff, (w >> 8) & 0xff, w >> 16
        k += 2 if opc == OP_S_ST8 else 1
        if opc in (OP_S_R1, OP_S_REP, OP_S_SPC, OP_S_ST8) and lo <= off < hi:
            assert off + (1 << stage) <= hi
            n += any(i not in fr for i in range(off, off + (1 << stage)))
    return n, virt


def test_codes_have_the_path_counts_meant():
    """N = 1024 (quarters recomputed): on the Bhattacharyya sets the first eighth is frozen and
    the second is not, so the G of quarter 0 runs with one path (P = 1: the lanes share the
    rounds) and the ops of quarter 1 with more; on the random sets the first eighth already
    branches (P > 1 at the G of quarter 0) and the first quarter holds at least log2 L branching leaves (P = L at the ops of quarter 1).
    N = 512: quarters stored, the staged ops are the root's children only."""
    from antpolarcodes_amd.rtc_codes import left_once_codes
    kinds = set()
    for c in left_once_codes():
        N, L, (kind, _), crc, sysm = c
        n8, virt = _branching_leaves(c, 0, N // 8)
        n4, _ = _branching_leaves(c, 0, N // 4)
        if N == 512:
            assert virt == 1
            continue
        assert N == 1024 and virt == 2
        if kind == "BB":
            info = [i for i in range(N // 4) if i not in set(_frozen(c))]
            assert info and min(info) >= N // 8 and n8 == 0 and n4 >= 1
        else:
            assert n8 >= 1 and 2 ** n4 >= L, (c[:2], n8, n4)
        kinds.add((L, kind == "BB", sysm))
    for L in (2, 4, 8):
        assert (L, True, True) in kinds and (L, False, True) in kinds
    assert (8, True, False) in kinds  # non-systematic
