"""The op classes of the specialised list kernel's walk, on the CPU (no GPU): the class table
and the per-position table that sclls_kernel.hip derives at compile time (ls_classify), read
back through pcg_dev_rtc_classes, which runs the same function on the host-only plan's schedule
and layout."""
import ctypes

import pytest

OP_F, OP_G, OP_S_ST8 = 1, 2, 44


def _list_codes():
    from antpolarcodes_amd.rtc_codes import codes
    return [c for c in codes() if c[1] > 1 and (len(c) == 5 or c[5] == "adaptive")]


def _id(c):
    N, L, (kind, arg), crc, sysm = c[:5]
    return f"N{N}-L{L}-{kind}{arg if kind != 'set' else len(arg)}-crc{crc}-{int(sysm)}" + "".join(f"-{v}" for v in c[5:])


def _plan(c):
    from antpolarcodes_amd._native import Plan
    from antpolarcodes_amd.construction import frozen_bits
    N, L, (kind, arg), crc, sysm = c[:5]
    fr = list(arg) if kind == "set" else frozen_bits(N, arg, 0.0, kind)
    return Plan(N, L, fr, systematic=sysm, crc=crc, device=-1, adaptive=len(c) > 5)


def _tables(p):
    from antpolarcodes_amd._native import lib
    ops = (ctypes.c_uint32 * 16384)()
    nops = lib().pcg_dev_plan_ops(p._h, ops, 16384)
    assert 0 < nops <= 16384
    keys = (ctypes.c_uint32 * 128)()
    pos = (ctypes.c_uint32 * (2 * nops))()
    ncls = ctypes.c_int(0)
    npos = lib().pcg_dev_rtc_classes(p._h, keys, 128, pos, nops, ctypes.byref(ncls))
    assert 0 < npos <= nops and 0 < ncls.value <= 128
    return list(ops[:nops]), list(keys[:ncls.value]), [(pos[2 * i], pos[2 * i + 1]) for i in range(npos)]


@pytest.mark.parametrize("code", _list_codes(), ids=_id)
def test_position_table_reexpands_to_the_schedule(code):
    """Codes, stages, offsets, descriptors and fused children of the per-position table, in
    order, are exactly the plan's schedule words; the classes are the distinct (code, stage,
    fused) triples of that walk, each once."""
    p = _plan(code)
    p.specialize()  # (from the shipped cache: the catalogue's kernels are built with the library)
    assert p.kernel_name() == "scl_rtc_kernel"
    ops, keys, pos = _tables(p)
    words, triples = [], set()
    for e, second in pos:
        cls, used, off = e & 0xff, (e >> 8) & 0xff, e >> 16
        assert cls < len(keys) and used in (1, 2)
        key = keys[cls]
        opc, stage, fused = key & 0xff, (key >> 8) & 0xff, (key >> 16) & 1
        assert key >> 17 == 0
        words.append(opc | stage << 8 | off << 16)
        assert used == (2 if fused or opc == OP_S_ST8 else 1)
        if used == 2:
            words.append(second)
        else:
            assert second == 0
        if fused:  # an F / G whose next schedule word is its child's F
            assert opc in (OP_F, OP_G) and second & 0xffff == (OP_F | (stage - 1) << 8)
        triples.add((opc, stage, fused))
    assert words == ops
    assert len(keys) == len(set(keys)) and len(keys) <= len(triples)
    assert {(k & 0xff, (k >> 8) & 0xff, (k >> 16) & 1) for k in keys} == triples
    p.close()


def test_class_codes_cover_the_derivation_branches():
    """tests/test_gpu_rtc_classes.py's codes are what it says: only the root's children recomputed up
    to N = 512, at N = 1024 the quarters too unless a leaf sits at stage top - 2 (both cases); fused
    F/G + F classes from N = 256 on and none at N = 32."""
    from antpolarcodes_amd.rtc_codes import class_codes
    virt, fused = {}, {}
    for c in class_codes():
        p = _plan(c)
        virt.setdefault(c[0], set()).add(p.describe()["recomputed_stages"])
        fused.setdefault(c[0], set()).add(any(k >> 16 & 1 for k in _tables(p)[1]))
        p.close()
    assert virt[32] == virt[64] == virt[256] == virt[512] == {1} and virt[1024] == {1, 2}, virt
    assert fused[32] == {False} and fused[256] == {True} and fused[1024] == {True}, fused


def test_config3_classes():
    """Config 3 (N = 1024, K = 512, L = 8): 280 schedule words, a few dozen classes."""
    p = _plan((1024, 8, ("BB", 512), 8, True))
    ops, keys, pos = _tables(p)
    assert len(ops) == 280 and len(keys) <= 40 and len(pos) < len(ops)
    p.close()


def test_knob_is_a_dev_build(monkeypatch):
    """PCG_RTC_CLASSES (the A/B switch between the per-class walk and the schedule loop) changes
    the generated source, hence the cache name, and marks the plan a development build."""
    from antpolarcodes_amd._native import lib
    names = {}
    for v in (None, "0", "1"):
        if v is None:
            monkeypatch.delenv("PCG_RTC_CLASSES", raising=False)
        else:
            monkeypatch.setenv("PCG_RTC_CLASSES", v)
        p = _plan((32, 2, ("BB", 16), 8, True))
        b = ctypes.create_string_buffer(256)
        assert lib().pcg_dev_rtc_cache_name(p._h, b, 256) == 0
        names[v] = b.value
        assert p.describe()["dev_overrides"] == (0 if v is None else 0x40)
        p.close()
    assert names[None] == names["1"] != names["0"]
