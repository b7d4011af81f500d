"""The compacted walk table of the specialised list kernel (sclls_kernel.hip ls_compact,
PCG_RTC_COMPACT), on the CPU: read back through pcg_dev_rtc_walk, which runs the kernel's own
constexpr passes on the host-only plan's schedule and layout.  Empty positions are left out, a run
of Combines up one node chain is one position, and (mode 2) a run and the G of its node's parent
are one position; the schedule itself is untouched, so every table re-expands to it."""
import ctypes

import pytest

from walk_table import (OP_COMB, OP_F, OP_G, PLAIN, RUN, RUN_G, WK_RUN, WK_RUNG, code_id, fg_empty, frozen_of,
                        host_plan, layout, walk, words_of)

DEFAULT_MODE = 1  # PCG_RTC_COMPACT unset, list widths <= 8: part 1 on, runs handed to their parent's G off


def _list_codes():
    """The catalogue's float list codes of at most 8 lanes per codeword (the per-class walk's), the
    GPU parity test's among them."""
    from antpolarcodes_amd.rtc_codes import codes, compact_codes
    out = [c for c in codes() if 1 < c[1] <= 8 and (len(c) == 5 or c[5] == "adaptive")]
    assert all(c in out for c in compact_codes())
    return out


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("code", _list_codes(), ids=code_id)
def test_table_is_the_schedule_once(code, mode):
    """Covered and dropped words, in order, are the schedule exactly once each; the dropped ones are
    exactly the unfused F and G words whose output stage the layout never stores (the rule computed
    here from describe()); a run is consecutive COMB words, stages rising by one and offsets
    falling by 2^s; a run + G has its G at the run's last stage + 1 and the run's last offset."""
    p = host_plan(code)
    top, mt, vlow, Sl = layout(p)
    w0, w = walk(p, 0), walk(p, mode)
    assert (w.mode, w.mt, w.vlow) == (mode, mt, vlow) and w.ops == w0.ops
    # mode 0 is ls_classify's table: one position per op, nothing dropped
    assert not w0.dropped and all(q.kind == PLAIN for q in w0.pos)
    assert [x for q in w0.pos for x in words_of(q)] == w0.ops
    expect_drop = [q.first for q in w0.pos
                   if q.code in (OP_F, OP_G) and not q.fused and fg_empty(q.stage, mt, vlow)]
    assert w.dropped == expect_drop
    # in order, each word once
    k, drop, words = 0, list(w.dropped), []
    for q in w.pos:
        while drop and drop[0] == k:
            words.append(w.ops[k])
            k += 1
            drop.pop(0)
        assert q.first == k, (q, k)
        mine = words_of(q)
        assert len(mine) == q.used
        words += mine
        k += q.used
    while drop and drop[0] == k:
        words.append(w.ops[k])
        k += 1
        drop.pop(0)
    assert not drop and k == len(w.ops) and words == w.ops
    for i, q in enumerate(w.pos):
        assert q.kind == {WK_RUN: RUN, WK_RUNG: RUN_G}.get(q.code, PLAIN)
        if q.kind == PLAIN:
            assert q.length == 0 and not (q.code in (OP_F, OP_G) and not q.fused and fg_empty(q.stage, mt, vlow))
            continue
        assert mode == 2 or q.kind == RUN
        last = q.stage + q.length - 1
        assert q.length >= (2 if q.kind == RUN else 1) and last <= 10 and q.off % (1 << last) == 0
        if q.kind == RUN_G:  # a stored, non-empty source stage of at most four bit words
            sg = last + 1
            assert sg < mt and sg <= 8 and (q.fused or not fg_empty(sg, mt, vlow))
            assert q.used == q.length + (2 if q.fused else 1) and bool(q.second) == bool(q.fused)
        else:
            assert q.used == q.length and not q.fused and q.second == 0
    # maximal: no Combine is left next to a run it continues (but for the register limit), and in
    # mode 2 no run or single Combine is left in front of a G it could have been handed to
    for a, b in zip(w.pos, w.pos[1:]):
        la = a.stage + max(a.length, 1) - 1
        if a.code in (OP_COMB, WK_RUN) and b.code == OP_COMB and b.stage == la + 1 and b.off + (1 << la) == a.off:
            assert b.stage > 10, (a, b)
        if mode == 2 and a.code in (OP_COMB, WK_RUN) and b.code == OP_G and b.stage == la + 1 and b.off == a.off:
            assert b.stage >= mt or b.stage > 8, (a, b)
    p.close()


def test_config3_counts():
    """Config 3 (N = 1024, K = 512, L = 8): 280 words in 242 positions; 52 of them empty (46 at
    stage 4, 6 at stages 9 and 10), 63 Combines in 33 runs, 16 of those single, 26 of the 33 in front
    of the parent's G at a stored stage (12 at stage 5, 8 at 6, 6 at 7, five of those fused with the
    child's F): 160 positions compacted, 134 with the runs handed on."""
    p = host_plan((1024, 8, ("BB", 512), 8, True))
    w0, w1, w2 = walk(p, 0), walk(p, 1), walk(p, 2)
    assert len(w0.ops) == 280 and len(w0.pos) == 242
    assert len(w1.dropped) == 52 and w1.dropped == w2.dropped
    st = [w0.ops[k] >> 8 & 0xff for k in w1.dropped]
    assert st.count(4) == 46 and st.count(9) + st.count(10) == 6
    assert sum(q.code == OP_COMB for q in w0.pos) == 63
    runs = [q for q in w1.pos if q.kind == RUN]
    singles = [q for q in w1.pos if q.code == OP_COMB]
    assert len(runs) == 17 and len(singles) == 16 and sum(q.length for q in runs) == 47
    assert len(w1.pos) == 242 - 52 - (47 - 17) == 160
    rg = [q for q in w2.pos if q.kind == RUN_G]
    assert len(rg) == 26 and {q.stage + q.length for q in rg} == {5, 6, 7}
    assert sum(q.fused for q in rg) == 5
    assert len(w2.pos) == 160 - 26 == 134
    p.close()


def _info_bits_before(code, end):
    fr = set(frozen_of(code))
    return sum(1 for i in range(end) if i not in fr)


def test_gpu_codes_hold_every_kind_of_position():
    """tests/test_gpu_rtc_compact.py's codes are what it says: N from 32 to 1024, at N = 1024 the
    quarters recomputed and stored, list sizes 2, 4, 5 and 8, one non-systematic; and among their
    walk positions a run within one word, one reaching the word XORs of stages 6 and 7, one over more
    than eight words, one ending the walk, one in front of an empty G, one in front of a recomputed
    quarter's G, run + G with the G reading LDS, reading the slab, and fused with its child's F,
    and a run + G reached with so few paths that the lanes share them (the run in the row, then the
    G reading it): the information bits decoded before the G bound the paths, 2^k, and the lanes
    share when twice that many still fit the lanes of a codeword."""
    from antpolarcodes_amd.rtc_codes import compact_codes
    cs = compact_codes()
    assert {c[0] for c in cs} >= {32, 64, 256, 512, 1024} and {c[1] for c in cs} == {2, 4, 5, 8}
    assert sum(not c[4] for c in cs) >= 1
    seen, virt = set(), set()
    for c in cs:
        p = host_plan(c)
        top, mt, vlow, Sl = layout(p)
        lp = p.describe()["lanes_per_codeword"]
        if c[0] == 1024:
            virt.add(p.describe()["recomputed_stages"])
        w1, w2 = walk(p, 1), walk(p, 2)
        for w in (w1, w2):
            for i, q in enumerate(w.pos):
                if q.kind == PLAIN:
                    continue
                last = q.stage + q.length - 1
                if last <= 5 and q.length >= 2:
                    seen.add("one word")
                if q.stage <= 6 and last >= 7:
                    seen.add("word xors 6, 7")
                if last >= 9:
                    seen.add("more than eight words")
                if i == len(w.pos) - 1 and q.first + q.used == len(w.ops):
                    seen.add("ends the walk")
                nxt = q.first + q.used
                if q.kind == RUN and nxt in w.dropped and w.ops[nxt] & 0xffff == (OP_G | (last + 1) << 8):
                    seen.add("before an empty G")
                if q.kind == RUN and i + 1 < len(w.pos):
                    g = w.pos[i + 1]
                    if g.code == OP_G and g.stage == last + 1 and g.off == q.off and mt <= g.stage <= top - 2:
                        seen.add("before a recomputed quarter's G")
                if q.kind == RUN_G:
                    sg = last + 1
                    seen.add("run + G fused" if q.fused else
                             "run + G from LDS" if Sl is not None and sg < Sl else "run + G from the slab")
                    k = _info_bits_before(c, q.off + (1 << last))
                    chunks = 1 << (sg - (4 if q.fused else 3))
                    if 2 * (1 << k) <= lp and chunks >= 4:
                        seen.add("run + G with shared paths")
                    if (1 << k) >= lp:
                        seen.add("run + G with a full list")
        p.close()
    assert virt == {1, 2}
    assert seen == {"one word", "word xors 6, 7", "more than eight words", "ends the walk", "before an empty G",
                    "before a recomputed quarter's G", "run + G fused", "run + G from LDS", "run + G from the slab",
                    "run + G with shared paths", "run + G with a full list"}, seen


def test_knob_is_a_dev_build(monkeypatch):
    """PCG_RTC_COMPACT (the A/B switch between the walk tables) changes the generated source, hence
    the cache name, and marks the plan a development build; unset it is the compacted table."""
    from antpolarcodes_amd._native import lib
    names, modes = {}, {}
    for v in (None, "0", "1", "2"):
        if v is None:
            monkeypatch.delenv("PCG_RTC_COMPACT", raising=False)
        else:
            monkeypatch.setenv("PCG_RTC_COMPACT", v)
        p = host_plan((32, 2, ("BB", 16), 8, True))
        b = ctypes.create_string_buffer(256)
        assert lib().pcg_dev_rtc_cache_name(p._h, b, 256) == 0
        names[v] = b.value
        modes[v] = walk(p).mode
        assert p.describe()["dev_overrides"] == (0 if v is None else 0x40)
        p.close()
    assert modes == {None: DEFAULT_MODE, "0": 0, "1": 1, "2": 2}
    assert names[None] == names[str(DEFAULT_MODE)] and len({names["0"], names["1"], names["2"]}) == 3
