"""GPU parity of the root's left child staged once per codeword (sclls_kernel.hip,
PCG_STG_LEFT_ONCE): the codeword's first staged op, the F of quarter 0, stores F(y_j, y_j+N/2)
into the wave's image, and the other staged ops of the left half -- the G of quarter 0, the F and
G of quarter 1 -- fetch it instead of the channel.  The interpreter kernel and the specialised
one against the oracle, bit for bit in info, ok and the ordered path metrics.

Codes (antpolarcodes_amd/rtc_codes.py left_once_codes; tests/test_left_once.py proves their
path counts on the CPU): N = 512 and 1024, L = 2, 4, 8; the Bhattacharyya sets freeze the first
eighth (config 3's own set: one path at both ops of quarter 0, the lanes sharing its rounds,
the writer unfused -- its child is a rate-0 leaf -- and more paths at quarter 1), the random sets
branch within the first eighth (P > 1 at the G of quarter 0, P = L at quarter 1); one
non-systematic.  12 frames per LLR family of helpers.LLR_KINDS (60 in all, the tie-heavy ones
included): never a multiple of the 8, 16 or 32 codewords of a wave.  Every code also runs on
the interpreter with the switch off (PCG_SCL_LEFT_ONCE=0: every op from the channel)."""
import numpy as np
import pytest

from helpers import LLR_KINDS, gpu_plan, llr_kinds

pytestmark = pytest.mark.gpu

FRAMES = 12

_cache = {}


def _codes():
    from antpolarcodes_amd.rtc_codes import left_once_codes
    return left_once_codes()


def _id(c):
    N, L, (kind, arg), crc, sysm = c
    return f"N{N}-L{L}-{kind}{arg if kind != 'set' else len(arg)}-crc{crc}-{'sys' if sysm else 'nonsys'}"


def _frozen(c):
    from antpolarcodes_amd.construction import frozen_bits
    N, L, (kind, arg), crc, sysm = c
    return list(arg) if kind == "set" else frozen_bits(N, arg, 0.0, kind)


def _case(oracle, c):
    """LLRs and the oracle's outputs of one code (computed once, shared, read-only)."""
    if c not in _cache:
        N, L, _, crc, sysm = c
        rng = np.random.default_rng(8200 + N + L + crc + int(sysm))
        llr = np.concatenate([llr_kinds(rng, FRAMES, N, k) for k in LLR_KINDS])
        oi, ook, om, _, _ = oracle.scl_decode(N, L, _frozen(c), llr, systematic=sysm, crc=crc, paths=True)
        for a in (llr, oi, ook, om):
            a.setflags(write=False)
        _cache[c] = (llr, oi, ook, om)
    return _cache[c]


def _same(got, exp, what):
    (gi, gok, gm), (oi, ook, om) = got, exp
    for k, name in enumerate(LLR_KINDS):
        sl = slice(k * FRAMES, (k + 1) * FRAMES)
        assert np.array_equal(gi[sl], oi[sl]), (what, name, "info")
        assert np.array_equal(gok[sl], ook[sl]), (what, name, "ok")
        assert np.array_equal(gm[sl].view(np.uint32), om[sl].view(np.uint32)), (what, name, "metrics")


@pytest.mark.parametrize("code", _codes(), ids=_id)
def test_matches_oracle_on_both_kernels(oracle, code):
    N, L, _, crc, sysm = code
    llr, oi, ook, om = _case(oracle, code)
    assert llr.shape[0] <= 64 and llr.shape[0] % (64 // max(2, 1 << (L - 1).bit_length())) != 0
    for kernel in ("rtc", "interp"):
        p = gpu_plan(N, L, _frozen(code), kernel=kernel, systematic=sysm, crc=crc)
        assert p.describe()["dev_overrides"] == 0
        _same(p.decode_host(llr, want_metrics=True), (oi, ook, om), kernel)
        p.close()


@pytest.mark.parametrize("code", _codes(), ids=_id)
def test_switch_off_matches_oracle(oracle, monkeypatch, code):
    """Every staged op from the channel (the walk before the image), on the interpreter."""
    monkeypatch.setenv("PCG_SCL_LEFT_ONCE", "0")
    N, L, _, crc, sysm = code
    llr, oi, ook, om = _case(oracle, code)
    p = gpu_plan(N, L, _frozen(code), kernel="interp", systematic=sysm, crc=crc)
    assert p.describe()["dev_overrides"] == 0x2
    _same(p.decode_host(llr, want_metrics=True), (oi, ook, om), "off")
    p.close()


def test_punctured_frames_use_the_image(oracle):
    """decode_punctured_device: the wave depunctures its group behind the images in its slab and
    the writer reads that copy (config 3's code, E = 896, 61 frames: a partial last group)."""
    import torch
    from antpolarcodes_amd._native import Puncturer
    E, N, K, L, F = 896, 1024, 512, 8, 61
    rng = np.random.default_rng(8300)
    fr = oracle.frozen_bits_bb(N, K, 0.0)
    llr = np.concatenate([llr_kinds(rng, 31, E, "normal"), llr_kinds(rng, F - 31, E, "ints")])
    dep = oracle.depuncture(E, fr, llr)
    oi, ook, om, _, _ = oracle.scl_decode(N, L, fr, dep, crc=8, paths=True)
    punc = Puncturer(E, fr, device=0)
    x = torch.from_numpy(llr).to("cuda:0")
    for kernel in ("interp", "rtc"):
        plan = gpu_plan(N, L, fr, kernel, crc=8)
        d_info = torch.empty((F, plan.kb), dtype=torch.uint8, device="cuda:0")
        d_ok = torch.empty(F, dtype=torch.uint8, device="cuda:0")
        d_met = torch.empty((F, L), dtype=torch.float32, device="cuda:0")
        plan.decode_punctured_device(punc, x, d_info, d_ok, d_met)
        torch.cuda.synchronize()
        assert np.array_equal(d_info.cpu().numpy(), oi), kernel
        assert np.array_equal(d_ok.cpu().numpy(), ook), kernel
        assert np.array_equal(d_met.cpu().numpy().view(np.uint32), om.view(np.uint32)), kernel
        plan.close()


@pytest.mark.parametrize("queue", ["1", "0"], ids=["queue", "static"])
@pytest.mark.parametrize("kernel", ["interp", "rtc"])
def test_image_is_rewritten_between_groups(oracle, monkeypatch, kernel, queue):
    """One list wave per CU (PCG_SCL_WPC = 1) and 8 (2 cus + 1) + 3 frames of config 3's code:
    every wave decodes two or three groups, so its images are rewritten between them, and the
    last group is partial.  The batch repeats 61 distinct frames (61 and the 8 cus frames between
    a wave's groups are coprime: no wave meets the same frames twice in a row)."""
    import torch
    monkeypatch.setenv("PCG_SCL_WPC", "1")
    if queue == "0":
        monkeypatch.setenv("PCG_SCL_QUEUE", "0")
    N, L, crc = 1024, 8, 8
    fr = oracle.frozen_bits_bb(N, 512, 0.0)
    rng = np.random.default_rng(8400)
    base = np.concatenate([llr_kinds(rng, 13 if k == "normal" else 12, N, k) for k in LLR_KINDS])
    assert base.shape[0] == 61
    oi, ook, om, _, _ = oracle.scl_decode(N, L, fr, base, crc=crc, paths=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    F = 8 * (2 * cus + 1) + 3
    rows = np.arange(F) % 61
    p = gpu_plan(N, L, fr, kernel=kernel, crc=crc)
    gi, gok, gm = p.decode_host(np.ascontiguousarray(base[rows]), want_metrics=True)
    p.close()
    assert np.array_equal(gi, oi[rows]) and np.array_equal(gok, ook[rows])
    assert np.array_equal(gm.view(np.uint32), om[rows].view(np.uint32))
