"""The codes of tests/test_gpu_rtc_streams.py, on the CPU (no GPU): each has the op classes whose
streaming helpers the test is about, read through pcg_dev_rtc_classes (the class table
sclls_kernel.hip derives at compile time), and their first information bits come early and late."""
import ctypes

import pytest

OP_F, OP_G = 1, 2


def _codes():
    from antpolarcodes_amd.rtc_codes import stream_codes
    return stream_codes()


def _id(c):
    N, L, (kind, arg), crc, sysm = c
    return f"N{N}-L{L}-{kind}{arg if kind != 'set' else len(arg)}-crc{crc}-{int(sysm)}"


def _frozen(c):
    from antpolarcodes_amd.construction import frozen_bits
    N, L, (kind, arg), crc, sysm = c
    return [int(v) for v in (arg if kind == "set" else frozen_bits(N, arg, 0.0, kind))]


def _keys(c):
    from antpolarcodes_amd._native import Plan, lib
    N, L, spec, crc, sysm = c
    p = Plan(N, L, _frozen(c), systematic=sysm, crc=crc, device=-1)
    ops = (ctypes.c_uint32 * 16384)()
    nops = lib().pcg_dev_plan_ops(p._h, ops, 16384)
    assert 0 < nops <= 16384
    keys = (ctypes.c_uint32 * 128)()
    pos = (ctypes.c_uint32 * (2 * nops))()
    ncls = ctypes.c_int(0)
    npos = lib().pcg_dev_rtc_classes(p._h, keys, 128, pos, nops, ctypes.byref(ncls))
    assert 0 < npos <= nops and 0 < ncls.value <= 128
    p.close()
    return {(k & 0xff, (k >> 8) & 0xff, (k >> 16) & 1) for k in keys[:ncls.value]}


@pytest.mark.parametrize("code", _codes(), ids=_id)
def test_stream_codes_have_the_slab_classes(code):
    """A fused F/G + F at stages 7 and 8 (ls_fgf from the slab, and from the recomputed stage
    above it) and an unfused F/G at stage 6, whose source is the slab: an op is only fused when
    its output stage is in the slab (ls_classify), so the fused stage-7 class puts stage 6 there."""
    keys = _keys(code)
    for s in (7, 8):
        assert any((op, s, 1) in keys for op in (OP_F, OP_G)), (s, sorted(keys))
    assert any((op, 6, 0) in keys for op in (OP_F, OP_G)), sorted(keys)


def test_stream_codes_first_information_bit_early_and_late():
    """Per block length: a code whose list starts to grow within the first 16 positions (a full
    list for nearly every op) and one where it stays a single path for more than N / 8 positions
    (the ops before it run with shared lanes); list sizes 2, 4 and 8 at both lengths, at most four
    codes new to the catalogue."""
    from antpolarcodes_amd.rtc_codes import bench_codes, class_codes, random_list_codes
    first = {}
    for c in _codes():
        fr = set(_frozen(c))
        first.setdefault(c[0], []).append(min(i for i in range(c[0]) if i not in fr))
    assert sorted(first) == [512, 1024]
    for N, v in first.items():
        assert min(v) < 16 and max(v) > N // 8, (N, v)
        assert {c[1] for c in _codes() if c[0] == N} == {2, 4, 8}
    old = {(c[0], c[1], tuple(c[2][1]) if c[2][0] == "set" else c[2], c[3], c[4]) for c in bench_codes() + class_codes()}
    old |= {(N, L, tuple(fr), 0, True) for N, L, fr in random_list_codes()}
    new = [c for c in _codes() if (c[0], c[1], tuple(c[2][1]) if c[2][0] == "set" else c[2], c[3], c[4]) not in old]
    assert len(new) <= 4, new


def test_knob_is_a_dev_build(monkeypatch):
    """PCG_RTC_STREAMS (the A/B switch of the literal streaming forms and their batch depths) changes
    the generated source, hence the cache name, and marks the plan a development build; the
    defaults spelled out give the default kernel's source but for the override lines."""
    from antpolarcodes_amd._native import Plan, lib
    from antpolarcodes_amd.construction import frozen_bits
    names = {}
    for v in (None, "0", "1,1,1,4,4"):
        if v is None:
            monkeypatch.delenv("PCG_RTC_STREAMS", raising=False)
        else:
            monkeypatch.setenv("PCG_RTC_STREAMS", v)
        p = Plan(32, 2, frozen_bits(32, 16, 0.0), systematic=True, crc=8, device=-1)
        b = ctypes.create_string_buffer(256)
        assert lib().pcg_dev_rtc_cache_name(p._h, b, 256) == 0
        names[v] = b.value
        assert p.describe()["dev_overrides"] == (0 if v is None else 0x40)
        p.close()
    assert len(set(names.values())) == 3
