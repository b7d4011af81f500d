"""The compacted walk table of the specialised list kernel (sclls_kernel.hip ls_compact), read
through pcg_dev_rtc_walk from a host-only plan, and the layout figures the tests derive on
their own from Plan.describe()."""
import ctypes
from collections import namedtuple

OP_F, OP_G, OP_COMB, OP_S_ST8 = 1, 2, 4, 44
WK_RUN, WK_RUNG = 0xf0, 0xf1
PLAIN, RUN, RUN_G = 0, 1, 2

Pos = namedtuple("Pos", "code stage fused length used off second first kind")
Walk = namedtuple("Walk", "ops keys pos dropped mode mt vlow")


def frozen_of(c):
    from antpolarcodes_amd.construction import frozen_bits
    N, L, (kind, arg), crc, sysm = c[:5]
    return list(arg) if kind == "set" else [int(v) for v in frozen_bits(N, arg, 0.0, kind)]


def host_plan(c):
    from antpolarcodes_amd._native import Plan
    N, L, _, crc, sysm = c[:5]
    return Plan(N, L, frozen_of(c), systematic=sysm, crc=crc, device=-1, adaptive=len(c) > 5)


def code_id(c):
    N, L, (kind, arg), crc, sysm = c[:5]
    return f"N{N}-L{L}-{kind}{arg if kind != 'set' else len(arg)}-crc{crc}-{'sys' if sysm else 'nonsys'}" + \
        "".join(f"-{v}" for v in c[5:])


def walk(p, mode=-1):
    """The walk table of plan p under PCG_RTC_COMPACT = mode (-1: the one its kernel is built with)."""
    from antpolarcodes_amd._native import lib
    ops = (ctypes.c_uint32 * 16384)()
    nops = lib().pcg_dev_plan_ops(p._h, ops, 16384)
    assert 0 < nops <= 16384
    keys = (ctypes.c_uint32 * 128)()
    pos = (ctypes.c_uint32 * (4 * nops))()
    drop = (ctypes.c_uint32 * nops)()
    info = (ctypes.c_uint32 * 4)()
    ncls = ctypes.c_int(0)
    npos = lib().pcg_dev_rtc_walk(p._h, mode, keys, 128, ctypes.byref(ncls), pos, nops, drop, nops, info)
    assert 0 < npos <= nops and 0 < ncls.value <= 128 and info[3] <= nops
    out = []
    for i in range(npos):
        e, second, first, kind = pos[4 * i:4 * i + 4]
        key = keys[e & 0xff]
        out.append(Pos(key & 0xff, (key >> 8) & 0xff, (key >> 16) & 1, key >> 24, (e >> 8) & 0xff, e >> 16, second,
                       first, kind))
    return Walk(list(ops[:nops]), list(keys[:ncls.value]), out, list(drop[:info[3]]), info[0], info[1], info[2])


def layout(p):
    """(top, first recomputed stage mt, recomputed low stages vlow, LDS stage limit Sl) of a list plan
    of at most 8 lanes per codeword, from describe() alone: the wave's LDS holds the LLR stages
    [3 + vlow, Sl), 64 * (2^Sl - 2^(3 + vlow)) floats, and the codeword rows, 64 words per 32 bits."""
    d = p.describe()
    assert d["lanes_per_codeword"] <= 8
    N = d["block_length"]
    top = N.bit_length() - 1
    mt = max(top - d["recomputed_stages"], 3)
    a = d["lds_bytes"] // 4 // 64 - max(1, N // 32)  # 2^Sl - 2^(3 + vlow)
    assert a >= 0
    if a == 0:  # no LLR stage in LDS: the layout's rule (stage 3 recomputed from N = 64 on)
        return top, mt, (1 if top >= 6 else 0), None
    low = (a & -a).bit_length() - 1
    Sl = (a + (1 << low)).bit_length() - 1
    assert (1 << Sl) - (1 << low) == a and low >= 3
    return top, mt, low - 3, Sl


def fg_empty(stage, mt, vlow):
    """An unfused F / G whose output stage is never stored: recomputed where it is read."""
    return stage - 1 >= mt or stage - 1 < 3 + vlow


def words_of(q):
    """The schedule words a walk position stands for."""
    w = []
    if q.kind == PLAIN:
        w.append(q.code | q.stage << 8 | q.off << 16)
    else:
        end = q.off + (1 << (q.stage + q.length - 1))  # every node of the run ends where the last one does
        for s in range(q.stage, q.stage + q.length):
            w.append(OP_COMB | s << 8 | (end - (1 << s)) << 16)
        if q.kind == RUN_G:
            w.append(OP_G | (q.stage + q.length) << 8 | q.off << 16)
    if q.second or q.code == OP_S_ST8:
        w.append(q.second)
    return w
