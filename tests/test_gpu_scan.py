"""The SCAN kernel (scan_kernel.hip) on the GPU, bit for bit against the reference's recorded
outputs (tests/golden/scan_fixtures.npz) and, where there is no fixture, against
tests/scan_numpy.py (pinned to the same fixtures by tests/test_scan_restatement.py).  Floats are
compared as their 32-bit patterns: +-0 and inf count."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits
from helpers import llr_kinds
from scan_numpy import scan_decode
from test_scan_restatement import fixture_cases, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "antpolarcodes_amd", "lib")
KINDS = ("ints", "zeros", "normal", "sparse", "wide")  # the tie-heavy families first: in every batch


def _nat():
    from antpolarcodes_amd import _native
    return _native


def mixed_llr(rng, F, N):
    """Frame f from family KINDS[f % 5]."""
    x = np.empty((F, N), np.float32)
    for k, kind in enumerate(KINDS):
        n = len(range(k, F, len(KINDS)))
        if n:
            x[k::len(KINDS)] = llr_kinds(rng, n, N, kind)
    return x


def check(got, want, tag, K=None):
    info, ok, soft, ext = got
    s, e, b = want[:3]
    assert same_bits(soft, s), (tag, "soft")
    assert same_bits(ext, e), (tag, "extrinsic")
    if K is not None and K % 8:
        assert np.array_equal(np.unpackbits(info, axis=1)[:, :K], np.unpackbits(b, axis=1)[:, :K]), (tag, "info")
    else:
        assert np.array_equal(info, b), (tag, "info")
    if len(want) > 3:
        assert np.array_equal(ok, want[3]), (tag, "ok")


def test_reference_fixtures():
    nat = _nat()
    for N, fr, it, sysm, llr, soft, ext, info, ok in fixture_cases():
        p = nat.ScanPlan(N, it, fr, systematic=sysm, crc=8)
        check(p.decode_host(llr), (soft, ext, info, ok), (N, it, sysm))
        p.close()


def test_known_answer_frame_through_pypolar():
    from antpolarcodes_amd import pypolar
    for N, fr, it, sysm, llr, soft, ext, info, ok in fixture_cases():
        if N != 8:
            continue
        dec = pypolar.ScanDecoder(8, it, fr)
        dec.setSystematic(sysm)
        # (K = 4: decode_vector returns infoLength() // 8 = 0 bytes, as the reference's binding)
        assert dec.decode_vector(llr[0]).size == 0
        assert same_bits(dec.getSoftCodeword(), soft[0]), (it, sysm)
        assert same_bits(dec.getExtrinsicChannelInformation(), ext[0]), (it, sysm)
        free = np.setdiff1d(np.arange(8), fr)
        assert same_bits(dec.getSoftInformation(), soft[0][free]), (it, sysm)


SHAPES = [(N, N // 2) for N in (8, 16, 32, 64, 128, 512, 2048, 4096)] + [(64, 1), (64, 63)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_shape_edges(N, K):
    """Partial lane groups, partial waves, more than one wave; 0 .. 5 iterations; both modes."""
    nat = _nat()
    fr = frozen_bits(N, K, 0.0)
    big = N >= 2048
    Fs = (1, 3, 63, 64, 65) if big else (1, 3, 63, 64, 65, 257)
    its = (2,) if big else (0, 1, 2, 5)
    llr = mixed_llr(np.random.default_rng(N + K), max(Fs), N)
    for sysm in (True, False):
        p = nat.ScanPlan(N, its[0], fr, systematic=sysm, crc=0)
        for it in its:
            p.set_iterations(it)
            want = scan_decode(N, fr, llr, it, sysm)
            if it == 0 and not sysm:  # a fresh decoder's outputs: +0
                want = (np.zeros_like(llr), want[1], np.zeros_like(want[2]))
            for F in Fs:
                check(p.decode_host(llr[:F]), tuple(w[:F] for w in want), (N, K, sysm, it, F), K)
        p.close()


@pytest.mark.parametrize("N", [64, 128])
def test_random_frozen_sets(N):
    """Pruning against arbitrary patterns."""
    nat = _nat()
    rng = np.random.default_rng(1000 + N)
    for _ in range(30):
        K = int(rng.integers(1, N))
        fr = sorted(rng.choice(N, N - K, replace=False).tolist())
        llr = mixed_llr(rng, 8, N)
        for sysm in (True, False):
            p = nat.ScanPlan(N, 3, fr, systematic=sysm, crc=0)
            check(p.decode_host(llr), scan_decode(N, fr, llr, 3, sysm), (N, fr, sysm), K)
            p.close()


@pytest.mark.parametrize("kind", [0, 8, 16, 32])
def test_detectors(kind, oracle):
    from antpolarcodes_amd import frames
    nat = _nat()
    N, fr = 1024, frozen_bits(1024, 512, 0.0)
    llr, _, _ = frames.awgn_frames(N, fr, 256, 2.0, crc=kind)
    want = scan_decode(N, fr, llr, 4, True)
    ok = np.array([int(oracle.crc(kind, row)) for row in want[2]], np.uint8)
    if kind:  # (the dummy detector passes every frame)
        assert 0 in ok and 1 in ok
    else:
        assert ok.all()
    p = nat.ScanPlan(N, 4, fr, crc=kind)
    check(p.decode_host(llr), want + (ok,), kind)


def test_no_state_is_carried():
    nat = _nat()
    N, fr = 256, frozen_bits(256, 128, 0.0)
    rng = np.random.default_rng(9)
    A, B = mixed_llr(rng, 70, N), mixed_llr(rng, 70, N) * np.float32(3.0)
    p = nat.ScanPlan(N, 3, fr, crc=8)
    a1, _, a2 = p.decode_host(A), p.decode_host(B), p.decode_host(A)
    for x, y in zip(a1, a2):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    check(a1, scan_decode(N, fr, A, 3, True), "A")
    # the iteration limit changed on one plan equals fresh plans
    q = nat.ScanPlan(N, 1, fr, crc=8)
    for it in (1, 4):
        q.set_iterations(it)
        got, fresh = q.decode_host(A), nat.ScanPlan(N, it, fr, crc=8).decode_host(A)
        for x, y in zip(got, fresh):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), it
        check(got, scan_decode(N, fr, A, it, True), it)
    # a larger batch after a small one: the slab and the staging grow
    big = mixed_llr(rng, 257, N)
    r = nat.ScanPlan(N, 2, fr, crc=8)
    check(r.decode_host(big[:3]), tuple(w[:3] for w in scan_decode(N, fr, big[:3], 2, True)), "F=3")
    check(r.decode_host(big), scan_decode(N, fr, big, 2, True), "F=257")


def test_device_path_and_untouched_outputs():
    import torch
    nat = _nat()
    N, fr, F = 512, frozen_bits(512, 256, 0.0), 130
    llr = mixed_llr(np.random.default_rng(4), F, N)
    s, e, b = scan_decode(N, fr, llr, 2, True)
    p = nat.ScanPlan(N, 2, fr, crc=8)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(llr).to(dev)
    stream = torch.cuda.Stream(device=dev)
    sentinel = 12345.0
    for want_soft, want_ext, want_ok in ((True, True, True), (False, True, True), (True, False, True),
                                         (False, False, False)):
        info = torch.full((F, p.kb), 0xAA, dtype=torch.uint8, device=dev)
        ok = torch.full((F,), 7, dtype=torch.uint8, device=dev)
        soft = torch.full((F, N), sentinel, dtype=torch.float32, device=dev)
        ext = torch.full((F, N), sentinel, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            p.decode_device(x, info, ok if want_ok else None, soft if want_soft else None,
                            ext if want_ext else None, stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(info.cpu().numpy(), b)
        if want_ok:
            assert set(ok.cpu().numpy().tolist()) <= {0, 1}
        else:
            assert (ok.cpu().numpy() == 7).all()
        assert same_bits(soft.cpu().numpy(), s) if want_soft else (soft.cpu().numpy() == sentinel).all()
        assert same_bits(ext.cpu().numpy(), e) if want_ext else (ext.cpu().numpy() == sentinel).all()
    # the info / ok and the soft-codeword forms of the generic entry points
    info = torch.zeros((F, p.kb), dtype=torch.uint8, device=dev)
    soft = torch.zeros((F, N), dtype=torch.float32, device=dev)
    nat.Plan.decode_device(p, x, info)
    torch.cuda.synchronize()
    assert np.array_equal(info.cpu().numpy(), b)
    nat.Plan.decode_soft_device(p, x, info, None, soft)
    torch.cuda.synchronize()
    assert same_bits(soft.cpu().numpy(), s)
    i2, _, s2 = nat.Plan.decode_soft_host(p, llr)
    assert np.array_equal(i2, b) and same_bits(s2, s)
    assert np.array_equal(nat.Plan.decode_host(p, llr)[0], b)


def test_host_path_across_a_chunk_boundary():
    """pcg_decode_scan_f32_host streams chunks of min(65536, max(4096, 64 MB / frame bytes)) frames
    (capi.cpp): N = 8 has the 65536-frame chunk; one frame more makes a second chunk."""
    nat = _nat()
    N, fr, F = 8, [0, 1, 2, 4], 65536 + 1
    rng = np.random.default_rng(2)
    llr = rng.integers(-6, 7, (F, N)).astype(np.float32)
    p = nat.ScanPlan(N, 2, fr, crc=0)
    check(p.decode_host(llr), scan_decode(N, fr, llr, 2, True), "chunk + 1", 4)


def test_decode_batch_equals_decode_vector(oracle):
    from antpolarcodes_amd import frames, pypolar
    N, fr = 256, frozen_bits(256, 128, 0.0)
    llr, _, _ = frames.awgn_frames(N, fr, 5, 1.0, seed=3, crc=8)
    dec = pypolar.ScanDecoder(N, 3, fr)
    info, ok, soft, ext = dec.decode_batch(llr, return_ok=True, return_soft=True, return_extrinsic=True)
    s, e, b = scan_decode(N, fr, llr, 3, True)
    assert same_bits(soft, s) and same_bits(ext, e) and np.array_equal(info, b)
    assert ok.tolist() == [int(oracle.crc(8, row)) for row in b]
    assert np.array_equal(dec.decode_batch(llr), b)
    free = np.setdiff1d(np.arange(N), fr)
    for f in range(5):
        assert np.array_equal(dec.decode_vector(llr[f]), b[f])
        assert same_bits(dec.getSoftCodeword(), s[f])
        assert same_bits(dec.getSoftInformation(), s[f][free])
        assert same_bits(dec.getExtrinsicChannelInformation(), e[f])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_single_frame_flow(tmp_path, oracle):
    """setSignal -> decode -> getSoftCodeword / getSoftInformation / getExtrinsicChannelInformation /
    getDecodedInformationBits of PolarCode::Decoding::Scan (tests/cpp/scan_caller.cpp)."""
    from antpolarcodes_amd import frames
    exe = str(tmp_path / "scan_caller")
    src = os.path.join(ROOT, "tests", "cpp", "scan_caller.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", LIB, "-lpolarcode_amd", "-lpcg", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    N, F, it = 1024, 3, 2
    fr = frozen_bits(N, 512, 0.0)
    llr, _, _ = frames.awgn_frames(N, fr, F, 1.5, seed=5, crc=8)
    (tmp_path / "frozen.txt").write_text(" ".join(str(v) for v in fr))
    (tmp_path / "llr.bin").write_bytes(np.ascontiguousarray(llr, np.float32).tobytes())
    r = subprocess.run([exe, "gpu", str(tmp_path / "frozen.txt"), str(tmp_path / "llr.bin"), str(F), str(it)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "scan gpu ok" in r.stdout
    s, e, b = scan_decode(N, fr, llr, it, True)
    free = np.setdiff1d(np.arange(N), fr)
    for f, line in enumerate(r.stdout.splitlines()[:F]):
        okv, info, soft, ext, sinfo = line.split()
        assert int(okv) == int(oracle.crc(8, b[f])), f
        assert np.array_equal(np.frombuffer(bytes.fromhex(info), np.uint8), b[f]), f
        assert same_bits(np.frombuffer(bytes.fromhex(soft), np.float32), s[f]), f
        assert same_bits(np.frombuffer(bytes.fromhex(ext), np.float32), e[f]), f
        assert same_bits(np.frombuffer(bytes.fromhex(sinfo), np.float32), s[f][free]), f
