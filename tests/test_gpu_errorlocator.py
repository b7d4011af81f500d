"""The error-locator kernel (errorlocator_kernel.hip) on the GPU, byte for byte against the
reference's recorded outputs (tests/golden/errorlocator_fixtures.npz) and, where there is no
fixture, against tests/errorlocator_numpy.py (pinned to the same fixtures by
tests/test_errorlocator_restatement.py).  Leaf values and decoded words are compared as bytes."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits
from errorlocator_numpy import MODES, default_desired, locate
from test_errorlocator_restatement import check, fixture_cases, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "antpolarcodes_amd", "lib")


def _nat():
    from antpolarcodes_amd import _native
    return _native


def noisy_pair(N, fr, F, sigma, seed):
    """(noisy BPSK scaled by 4, the noiseless +-1 signal) of F non-systematic codewords."""
    from antpolarcodes_amd import frames
    x = frames.awgn_frames(N, fr, F, 2.0, seed=seed, crc=0, systematic=False)[2]
    clean = (1.0 - 2.0 * x.astype(np.float32)).astype(np.float32)
    noise = np.random.default_rng(seed + 1000).standard_normal((F, N)).astype(np.float32)
    return (np.float32(4.0) * (clean + np.float32(sigma) * noise)).astype(np.float32), clean


def test_reference_fixtures():
    """Every recorded case in all three modes: N = 8 (the size-8 op only), 16 (one RateR over two
    size-8 ops), 32, 64, 256 and 1024; every LLR kind against the defaults, AWGN frames against the
    reference-mode output of the clean signal, arbitrary desired vectors, K = N - 1."""
    nat = _nat()
    n, Ns = 0, set()
    for i, N, fr, llr, des, out in fixture_cases():
        p = nat.ErrorLocatorPlan(N, fr)
        assert p.kernel_name() == "errorlocator_kernel"
        for mode in MODES:
            check(p.locate_host(llr, des, mode, want_u=True, want_bits=True), out[mode], (i, N, mode))
        p.close()
        Ns.add(N)
        n += 1
    assert n >= 30 and {8, 16, 32, 64, 256, 1024} <= Ns


@pytest.mark.parametrize("N,K", [(8, 4), (64, 32), (256, 128)])
def test_shape_edges(N, K):
    """F = 1, 63, 65, 130: partial waves and more than one wave."""
    nat = _nat()
    fr = frozen_bits(N, K, 0.0)
    noisy, clean = noisy_pair(N, fr, 130, 1.0, seed=N)
    des = locate(N, fr, clean, None, "reference")[0]
    want = {m: locate(N, fr, noisy, des, m) for m in MODES}
    assert want["correct"][3].max() > 1 and (want["correct"][3] == 0).any()
    p = nat.ErrorLocatorPlan(N, fr)
    for F in (1, 63, 65, 130):
        for m in MODES:
            check(p.locate_host(noisy[:F], des[:F], m, want_bits=True), tuple(w[:F] for w in want[m]), (N, F, m))


def test_largest_block_length():
    """(4096, 2048) at F = 65: every level of the slab, two waves."""
    nat = _nat()
    N, K, F = 4096, 2048, 65
    fr = frozen_bits(N, K, 0.0)
    noisy, clean = noisy_pair(N, fr, F, 1.0, seed=9)
    p = nat.ErrorLocatorPlan(N, fr)
    des = p.locate_host(clean, None, "reference")[0]
    assert same(des, locate(N, fr, clean, None, "reference")[0])
    want = locate(N, fr, noisy, des, "correct")
    assert want[3].max() >= 64
    check(p.locate_host(noisy, des, "correct", want_bits=True), want, "4096")


def mixed_wave():
    """One wave's worth of (256, 128) frames with 0, 1 and many corrections."""
    N, K = 256, 128
    fr = frozen_bits(N, K, 0.0)
    parts = [noisy_pair(N, fr, 24, s, seed=int(100 * s)) for s in (0.3, 1.0, 1.6)]
    noisy, clean = (np.concatenate([p[k] for p in parts]) for k in (0, 1))
    des = locate(N, fr, clean, None, "reference")[0]
    # a lane with exactly one correction: its own reference output, one information sign flipped
    own = locate(N, fr, noisy[:1], None, "reference")[0]
    own[0, [i for i in range(N) if i not in set(fr)][-1]] *= -1
    noisy, des = np.concatenate([noisy[:63], noisy[:1]]), np.concatenate([des[:63], own])
    want = locate(N, fr, noisy, des, "correct")
    c = want[3]
    assert noisy.shape[0] == 64 and (c == 0).any() and (c == 1).any() and c.max() >= 32
    return N, fr, noisy, des, want


def test_one_wave_mixes_lanes_and_each_keeps_its_own_outputs():
    nat = _nat()
    N, fr, noisy, des, want = mixed_wave()
    p = nat.ErrorLocatorPlan(N, fr)
    check(p.locate_host(noisy, des, "correct", want_bits=True), want, "mix")
    # the same lanes in another order and spread over two waves
    perm = np.random.default_rng(1).permutation(np.tile(np.arange(64), 2))
    check(p.locate_host(noisy[perm], des[perm], "correct", want_bits=True), tuple(w[perm] for w in want), "two waves")


def test_optional_outputs_and_the_device_pointer_path():
    """Each output left NULL leaves the others unchanged and its buffer untouched; torch tensors on
    a side stream give the bytes of the host-pointer call."""
    import torch
    nat = _nat()
    N, fr, noisy, des, want = mixed_wave()
    p = nat.ErrorLocatorPlan(N, fr)
    u1, b1, f1, c1 = p.locate_host(noisy, des, "correct", want_u=False, want_bits=False)
    assert u1 is None and b1 is None and same(f1, want[2]) and same(c1, want[3])
    dev = torch.device("cuda:0")
    x, d = torch.from_numpy(noisy).to(dev), torch.from_numpy(des).to(dev)
    stream = torch.cuda.Stream(device=dev)
    F = noisy.shape[0]
    for wu, wb, wf, wc in itertools.product((True, False), repeat=4):
        u = torch.full((F, N), 7.0, dtype=torch.float32, device=dev)
        bits = torch.full((F, N), 12345, dtype=torch.int32, device=dev)
        first = torch.full((F,), 77, dtype=torch.int32, device=dev)
        count = torch.full((F,), 78, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            p.locate(x, d, "correct", u if wu else None, bits if wb else None, first if wf else None,
                     count if wc else None, stream=stream.cuda_stream)
        stream.synchronize()
        assert same(u.cpu().numpy(), want[0]) if wu else (u.cpu().numpy() == 7.0).all()
        assert same(bits.cpu().numpy(), want[1]) if wb else (bits.cpu().numpy() == 12345).all()
        assert same(first.cpu().numpy(), want[2]) if wf else (first.cpu().numpy() == 77).all()
        assert same(count.cpu().numpy(), want[3]) if wc else (count.cpu().numpy() == 78).all()


def test_no_desired_vector_is_the_default_vector():
    nat = _nat()
    from helpers import LLR_KINDS, llr_kinds
    rng = np.random.default_rng(8)
    for N, K in ((16, 8), (64, 40)):
        fr = frozen_bits(N, K, 0.0)
        llr = np.concatenate([llr_kinds(rng, 3, N, k) for k in LLR_KINDS])
        p = nat.ErrorLocatorPlan(N, fr)
        for m in MODES:
            a = p.locate_host(llr, None, m, want_bits=True)
            check(a, p.locate_host(llr, default_desired(N, fr, llr.shape[0]), m, want_bits=True), (N, m))
            check(a, locate(N, fr, llr, None, m), (N, m, "numpy"))


def test_host_path_across_a_chunk_boundary():
    """N = 8 has the 65536-frame chunk; one frame more makes a second chunk."""
    nat = _nat()
    N, fr, F = 8, [0, 1, 2, 4], 65536 + 1
    rng = np.random.default_rng(2)
    llr, des = rng.normal(0, 2, (F, N)).astype(np.float32), rng.normal(0, 2, (F, N)).astype(np.float32)
    check(nat.ErrorLocatorPlan(N, fr).locate_host(llr, des, "correct", want_bits=True), locate(N, fr, llr, des),
          "chunk + 1")


def test_pypolar_error_locator():
    from antpolarcodes_amd import pypolar
    N, fr, noisy, des, want = mixed_wave()
    el = pypolar.ErrorLocator(N, fr)
    u, bits, first, count = el.locate_batch(noisy, des, mode="correct", return_bits=True)
    check((u, bits, first, count), want, "locate_batch")
    u2, b2, f2, c2 = el.locate_batch(noisy, des, "first", return_u=False)
    assert u2 is None and b2 is None and same(f2, want[2]) and (c2 == 0).all()
    # the tool's single-frame flow
    ref = pypolar.ErrorLocator(N, fr)
    ref.setAsReferenceDecoder()
    for f in (0, 40, 63):
        el.setDesiredOutput(des[f])
        assert el.decode_vector(noisy[f]) is True
        assert (el.firstError(), el.correctionCount()) == (int(want[2][f]), int(want[3][f]))
        assert same(el.getOutput(), want[0][f]) and same(el.getSoftCodeword(), want[1][f])
        assert el.decodeFindFirstError(noisy[f]) == int(want[2][f]) and el.correctionCount() == 0
    assert ref.decode_vector(noisy[0]) is True
    assert same(ref.getOutput(), locate(N, fr, noisy[:1], None, "reference")[0][0])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_tool_flow_and_locate_batch(tmp_path):
    """The reference tool's flow through PolarCode::Decoding::ErrorLocator, then locateBatch
    (tests/cpp/errorlocator_caller.cpp)."""
    exe = str(tmp_path / "errorlocator_caller")
    src = os.path.join(ROOT, "tests", "cpp", "errorlocator_caller.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", LIB, "-lpolarcode_amd", "-lpcg", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    N, F = 1024, 4
    fr = frozen_bits(N, 512, 0.0)
    noisy, clean = noisy_pair(N, fr, F, 0.9, seed=5)
    (tmp_path / "frozen.txt").write_text(" ".join(str(v) for v in fr))
    (tmp_path / "clean.bin").write_bytes(clean.tobytes())
    (tmp_path / "noisy.bin").write_bytes(noisy.tobytes())
    r = subprocess.run([exe, "gpu", str(tmp_path / "frozen.txt"), str(tmp_path / "clean.bin"),
                        str(tmp_path / "noisy.bin"), str(F), str(N)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "errorlocator gpu ok" in r.stdout
    des = locate(N, fr, clean, None, "reference")[0]
    want = locate(N, fr, noisy, des, "correct")
    assert want[3].max() > 0
    lines = r.stdout.splitlines()
    for f, line in enumerate(lines[:F]):
        ret, first, count, u, words, ff = line.split()
        assert (int(ret), int(first), int(count), int(ff)) == (1, int(want[2][f]), int(want[3][f]), int(want[2][f]))
        assert same(np.frombuffer(bytes.fromhex(u), np.float32), want[0][f]), f
        assert same(np.frombuffer(bytes.fromhex(words), np.uint32), want[1][f]), f
    u, bits, first, count = (bytes.fromhex(v) for v in lines[F].split())
    check((np.frombuffer(u, np.float32).reshape(F, N), np.frombuffer(bits, np.uint32).reshape(F, N),
           np.frombuffer(first, np.int32), np.frombuffer(count, np.uint32)), want, "locateBatch")


def test_simulator_counts_equal_the_restatement_on_the_same_frames():
    """errorlocator -n 256 -r 0.5 -s 2 -w 2048: the histogram and the per-position count lists equal
    what the restatement yields on the very same LLRs and desired values."""
    from antpolarcodes_amd import errorlocator as tool
    seen = []
    job = tool.Job(tool.parser().parse_args(["-n", "256", "-r", "0.5", "-s", "2.0", "-w", "2048"]))
    tool.run(job, batch=1024, make_backend=lambda w: tool.GpuBackend(0, hook=lambda llr, des: seen.append(
        (llr.cpu().numpy(), des.cpu().numpy()))))
    assert job.runs == 2048 and len(seen) == 2
    hist, lists = np.zeros(256, np.int64), [[] for _ in range(256)]
    for llr, des in seen:
        assert (np.abs(des[:, job.frozenSet]) == np.inf).all()
        _, _, first, count = locate(256, job.frozen, llr, des, "correct")
        for f in np.flatnonzero(count > 0):
            hist[first[f]] += 1
            lists[first[f]].append(float(count[f]))
    assert np.array_equal(job.firstErrorPosition, hist) and job.additionalErrors == lists
    assert 0 < hist.sum() < 2048 and not hist[job.frozenSet].any()
