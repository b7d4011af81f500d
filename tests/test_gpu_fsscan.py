"""The Fast-SSCAN kernel (fsscan_kernel.hip) on the GPU, bit for bit against the reference's
recorded outputs (tests/golden/fsscan_fixtures.npz) and, where there is no fixture, against
tests/fsscan_numpy.py (pinned to the same fixtures by tests/test_fsscan_restatement.py).  Floats
are compared as their 32-bit patterns: +-0 and inf count."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits
from fsscan_numpy import fsscan_census, fsscan_decode
from helpers import llr_kinds
from test_fsscan_restatement import checker, fixture_cases
from test_scan_restatement import same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "antpolarcodes_amd", "lib")
KINDS = ("ints", "zeros", "normal", "sparse", "wide")  # the tie-heavy families first: in every batch


def _nat():
    from antpolarcodes_amd import _native
    return _native


def mixed_llr(rng, F, N, fr=None):
    """Frame f from family KINDS[f % 5]; with `fr`, the "normal" frames are CRC-8 codewords
    through AWGN at 2 dB, so that some frames of every wave pass their check early."""
    x = np.empty((F, N), np.float32)
    for k, kind in enumerate(KINDS):
        n = len(range(k, F, len(KINDS)))
        if n and kind == "normal" and fr is not None:
            from antpolarcodes_amd import frames
            x[k::len(KINDS)] = frames.awgn_frames(N, fr, n, 2.0, seed=N + F, crc=8)[0]
        elif n:
            x[k::len(KINDS)] = llr_kinds(rng, n, N, kind)
    return x


def check(got, want, tag, K=None):
    """got = (info, ok, soft, trials) of the plan, want = (soft, info, ok, trials) of the checker."""
    info, ok, soft, trials = got
    s, b, k, t = want
    assert np.array_equal(trials, t), (tag, "trials")
    assert np.array_equal(ok, k), (tag, "ok")
    assert same_bits(soft, s), (tag, "soft")
    if K is not None and K % 8:
        assert np.array_equal(np.unpackbits(info, axis=1)[:, :K], np.unpackbits(b, axis=1)[:, :K]), (tag, "info")
    else:
        assert np.array_equal(info, b), (tag, "info")


def test_reference_fixtures(oracle):
    """Every recorded case whose frames are independent; of the two recorded from one reused
    reference decoder (a right-child TwoBit node carries its message over there), the first
    frame, and all frames against the zero-start restatement."""
    nat = _nat()
    n = 0
    for N, fr, limit, crc, again, reused, llr, soft, info, ok, trials in fixture_cases():
        p = nat.FastSscanPlan(N, limit, fr, crc=crc)
        if again:
            p.set_trials(limit + again, forced=True)
        got = p.decode_host(llr)
        if reused:
            check(tuple(g[:1] for g in got), (soft[:1], info[:1], ok[:1], trials[:1]), (N, limit, crc, "frame 0"))
            check(got, fsscan_decode(N, fr, llr, limit, checker(oracle, crc)), (N, limit, crc, "zero start"))
        else:
            check(got, (soft, info, ok, trials), (N, limit, crc, again))
        p.close()
        n += 1
    assert n >= 21


def test_known_answer_frame_through_pypolar():
    from antpolarcodes_amd import pypolar
    kat = {again: soft for N, _, _, _, again, _, _, soft, *_ in fixture_cases() if N == 8}
    assert sorted(kat) == [0, 1]
    dec = pypolar.FastSscanDecoder(8, 1, [0, 1, 2, 4])
    dec.setErrorDetection(0)
    llr = np.array([-5, -6, -4, 1, -4, -5, -7, 2], np.float32)
    # (K = 4: decode_vector returns infoLength() // 8 = 0 bytes, as the reference's binding)
    assert dec.decode_vector(llr).size == 0 and dec.trials() == 1
    assert same_bits(dec.getSoftCodeword(), kat[0][0])
    assert same_bits(dec.getSoftInformation(), kat[0][0][[3, 5, 6, 7]])
    assert dec.decodeAgain() is True and dec.trials() == 2
    assert same_bits(dec.getSoftCodeword(), kat[1][0])
    assert dec.decode_vector(llr).size == 0 and dec.trials() == 1  # a new decode starts over
    assert same_bits(dec.getSoftCodeword(), kat[0][0])


SHAPES = [(N, N // 2) for N in (8, 16, 32, 64, 128, 512, 2048, 4096)] + [(64, 1), (64, 63)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_shape_edges(oracle, N, K):
    """Partial lane groups, partial waves, more than one wave; limits 1, 2, 5, forced and not;
    without a detector (every frame stops after pass 1) and with CRC-8."""
    nat = _nat()
    fr = frozen_bits(N, K, 0.0)
    Fs = (1, 3, 63, 64, 65) if N >= 2048 else (1, 3, 63, 64, 65, 257)
    llr = mixed_llr(np.random.default_rng(N + K), max(Fs), N, fr if K >= 16 else None)
    for crc in (0, 8):
        p = nat.FastSscanPlan(N, 1, fr, crc=crc)
        for limit in (1, 2, 5):
            for forced in (False, True):
                p.set_trials(limit, forced)
                want = fsscan_decode(N, fr, llr, limit, checker(oracle, crc), forced=forced)
                if not forced and not crc:
                    assert (want[3] == 1).all()
                if not forced and crc and K >= 16:  # frames that stop early and frames that do not
                    assert want[3].min() == 1 and want[3].max() == limit
                for F in Fs:
                    check(p.decode_host(llr[:F]), tuple(w[:F] for w in want), (N, K, crc, limit, forced, F), K)
        p.close()


def test_early_stop_mix(oracle):
    """Lanes of one wave stop at different passes: BB (256, 128), CRC-8, limit 4, 200 frames in
    their generated order.  Each lane keeps the outputs of the pass it passed in."""
    from antpolarcodes_amd import frames
    nat = _nat()
    N, fr = 256, frozen_bits(256, 128, 0.0)
    llr, _, _ = frames.awgn_frames(N, fr, 200, 1.0, seed=7, crc=8)
    want = fsscan_decode(N, fr, llr, 4, checker(oracle, 8))
    counts = np.bincount(want[3], minlength=5)
    print("passes run 1..4:", counts[1:].tolist())
    assert (counts[1:] > 0).all() and counts[1] >= 10 and counts[4] >= 10 and counts[0] == 0
    assert 0 in want[2] and 1 in want[2]
    for w0 in range(0, 200, 64):  # every wave has lanes that stop early and lanes that do not
        assert len(set(want[3][w0:w0 + 64].tolist())) >= 2
    p = nat.FastSscanPlan(N, 4, fr, crc=8)
    check(p.decode_host(llr), want, "mix")
    # ... and without the soft output, whose stores the same predicate guards
    info, ok, _, trials = p.decode_host(llr, want_soft=False)
    assert np.array_equal(info, want[1]) and np.array_equal(ok, want[2]) and np.array_equal(trials, want[3])


def random_sets(N):
    rng = np.random.default_rng(1000 + N)
    for _ in range(30):
        K = int(rng.integers(1, N))
        yield K, sorted(rng.choice(N, N - K, replace=False).tolist()), rng


@pytest.mark.parametrize("N", [64, 128])
def test_random_frozen_sets(oracle, N):
    """Arbitrary patterns against the zero-start restatement, sets with a TwoBit node that is a
    right child among them."""
    nat = _nat()
    right_twobit = 0
    for K, fr, rng in random_sets(N):
        llr = mixed_llr(rng, 8, N)
        right_twobit += fsscan_census(N, fr)["right_twobit"] > 0
        for crc, limit, forced in ((0, 3, True), (8, 3, False)):
            if crc >= K:
                continue
            p = nat.FastSscanPlan(N, limit, fr, crc=crc)
            p.set_trials(limit, forced)
            check(p.decode_host(llr), fsscan_decode(N, fr, llr, limit, checker(oracle, crc), forced=forced),
                  (N, fr, crc), K)
            p.close()
    assert right_twobit > 0


def test_no_state_is_carried(oracle):
    nat = _nat()
    N = 64
    fr = next(f for _, f, _ in random_sets(N) if fsscan_census(N, f)["right_twobit"] > 0)
    rng = np.random.default_rng(9)
    A, B = mixed_llr(rng, 70, N), mixed_llr(rng, 70, N) * np.float32(3.0)
    chk = checker(oracle, 8)
    # on this set a reused reference decoder gives other outputs than a fresh one per frame
    assert not same_bits(fsscan_decode(N, fr, A, 3, chk, carry=True)[0], fsscan_decode(N, fr, A, 3, chk)[0])
    p = nat.FastSscanPlan(N, 3, fr, crc=8)
    a1, _, a2 = p.decode_host(A), p.decode_host(B), p.decode_host(A)
    for x, y in zip(a1, a2):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    check(a1, fsscan_decode(N, fr, A, 3, chk), "A")
    # the limit changed on one plan equals fresh plans
    q = nat.FastSscanPlan(N, 1, fr, crc=8)
    for limit, forced in ((1, False), (4, False), (2, True), (1, False)):
        q.set_trials(limit, forced)
        fresh = nat.FastSscanPlan(N, limit, fr, crc=8)
        fresh.set_trials(limit, forced)
        got = q.decode_host(A)
        for x, y in zip(got, fresh.decode_host(A)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), limit
        check(got, fsscan_decode(N, fr, A, limit, chk, forced=forced), (limit, forced))
    # a larger batch after a small one: the slab and the staging grow
    big = mixed_llr(rng, 257, N)
    r = nat.FastSscanPlan(N, 2, fr, crc=8)
    want = fsscan_decode(N, fr, big, 2, chk)
    check(r.decode_host(big[:3]), tuple(w[:3] for w in want), "F=3")
    check(r.decode_host(big), want, "F=257")


@pytest.mark.parametrize("kind", [0, 8, 16, 32])
def test_detectors(kind, oracle):
    from antpolarcodes_amd import frames
    nat = _nat()
    N, fr = 1024, frozen_bits(1024, 512, 0.0)
    llr, _, _ = frames.awgn_frames(N, fr, 256, 2.0, crc=kind)
    want = fsscan_decode(N, fr, llr, 3, checker(oracle, kind))
    if kind:  # (the dummy detector passes every frame)
        assert 0 in want[2] and 1 in want[2]
    else:
        assert want[2].all() and (want[3] == 1).all()
    p = nat.FastSscanPlan(N, 3, fr, crc=kind)
    check(p.decode_host(llr), want, kind)


def test_device_path_and_untouched_outputs(oracle):
    import itertools
    import torch
    nat = _nat()
    N, fr, F = 512, frozen_bits(512, 256, 0.0), 130
    llr = mixed_llr(np.random.default_rng(4), F, N, fr)
    s, b, k, t = fsscan_decode(N, fr, llr, 2, checker(oracle, 8))
    assert len(set(t.tolist())) == 2
    p = nat.FastSscanPlan(N, 2, fr, crc=8)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(llr).to(dev)
    stream = torch.cuda.Stream(device=dev)
    sentinel = 12345.0
    for want_ok, want_soft, want_trials in itertools.product((True, False), repeat=3):
        info = torch.full((F, p.kb), 0xAA, dtype=torch.uint8, device=dev)
        ok = torch.full((F,), 7, dtype=torch.uint8, device=dev)
        trials = torch.full((F,), 77, dtype=torch.uint8, device=dev)
        soft = torch.full((F, N), sentinel, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            p.decode_device(x, info, ok if want_ok else None, soft if want_soft else None,
                            trials if want_trials else None, stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(info.cpu().numpy(), b)
        assert np.array_equal(ok.cpu().numpy(), k) if want_ok else (ok.cpu().numpy() == 7).all()
        assert np.array_equal(trials.cpu().numpy(), t) if want_trials else (trials.cpu().numpy() == 77).all()
        assert same_bits(soft.cpu().numpy(), s) if want_soft else (soft.cpu().numpy() == sentinel).all()
    # frames that start 4 bytes into an allocation: the kernel's other way of reading them
    y = torch.zeros(F * N + 1, dtype=torch.float32, device=dev)[1:].view(F, N)
    y.copy_(x)
    assert y.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    info = torch.zeros((F, p.kb), dtype=torch.uint8, device=dev)
    ok = torch.zeros((F,), dtype=torch.uint8, device=dev)
    soft = torch.zeros((F, N), dtype=torch.float32, device=dev)
    trials = torch.zeros((F,), dtype=torch.uint8, device=dev)
    p.decode_device(y, info, ok, soft, trials)
    torch.cuda.synchronize()
    check((info.cpu().numpy(), ok.cpu().numpy(), soft.cpu().numpy(), trials.cpu().numpy()), (s, b, k, t), "offset")
    # the info / ok and the soft-codeword forms of the generic entry points
    info.zero_(), ok.zero_(), soft.zero_()
    nat.Plan.decode_device(p, x, info, ok)
    torch.cuda.synchronize()
    assert np.array_equal(info.cpu().numpy(), b) and np.array_equal(ok.cpu().numpy(), k)
    nat.Plan.decode_soft_device(p, x, info, None, soft)
    torch.cuda.synchronize()
    assert same_bits(soft.cpu().numpy(), s)
    i2, k2, s2 = nat.Plan.decode_soft_host(p, llr)
    assert np.array_equal(i2, b) and np.array_equal(k2, k) and same_bits(s2, s)
    assert np.array_equal(nat.Plan.decode_host(p, llr)[0], b)


def test_host_path_across_a_chunk_boundary():
    """pcg_decode_fsscan_f32_host streams chunks of min(65536, max(4096, 64 MB / frame bytes))
    frames (capi.cpp): N = 8 has the 65536-frame chunk; one frame more makes a second chunk."""
    nat = _nat()
    N, fr, F = 8, [0, 1, 2, 4], 65536 + 1
    rng = np.random.default_rng(2)
    llr = rng.integers(-6, 7, (F, N)).astype(np.float32)
    p = nat.FastSscanPlan(N, 2, fr, crc=0)
    p.set_trials(2, forced=True)
    check(p.decode_host(llr), fsscan_decode(N, fr, llr, 2, forced=True), "chunk + 1", 4)


def test_decode_batch_equals_decode_vector(oracle):
    from antpolarcodes_amd import frames, pypolar
    N, fr = 256, frozen_bits(256, 128, 0.0)
    llr, _, _ = frames.awgn_frames(N, fr, 6, 1.0, seed=3, crc=8)
    dec = pypolar.FastSscanDecoder(N, 3, fr)
    info, ok, soft, trials = dec.decode_batch(llr, return_ok=True, return_soft=True, return_trials=True)
    s, b, k, t = fsscan_decode(N, fr, llr, 3, checker(oracle, 8))
    assert same_bits(soft, s) and np.array_equal(info, b) and np.array_equal(ok, k) and np.array_equal(trials, t)
    assert np.array_equal(dec.decode_batch(llr), b)
    free = np.setdiff1d(np.arange(N), fr)
    for f in range(6):
        assert np.array_equal(dec.decode_vector(llr[f]), b[f])
        assert dec.trials() == t[f]
        assert same_bits(dec.getSoftCodeword(), s[f])
        assert same_bits(dec.getSoftInformation(), s[f][free])
        nxt = fsscan_decode(N, fr, llr[f:f + 1], int(t[f]) + 1, checker(oracle, 8), forced=True)
        assert dec.decodeAgain() == bool(nxt[2][0])
        assert same_bits(dec.getSoftCodeword(), nxt[0][0])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_single_frame_flow(tmp_path, oracle):
    """setSignal -> decode -> getSoftCodeword / getSoftInformation -> decodeAgain -> getSoftCodeword
    of PolarCode::Decoding::FastSscanFloat (tests/cpp/fsscan_caller.cpp)."""
    from antpolarcodes_amd import frames
    exe = str(tmp_path / "fsscan_caller")
    src = os.path.join(ROOT, "tests", "cpp", "fsscan_caller.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", LIB, "-lpolarcode_amd", "-lpcg", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    N, F, limit = 1024, 3, 2
    fr = frozen_bits(N, 512, 0.0)
    llr, _, _ = frames.awgn_frames(N, fr, F, 1.5, seed=5, crc=8)
    (tmp_path / "frozen.txt").write_text(" ".join(str(v) for v in fr))
    (tmp_path / "llr.bin").write_bytes(np.ascontiguousarray(llr, np.float32).tobytes())
    r = subprocess.run([exe, "gpu", str(tmp_path / "frozen.txt"), str(tmp_path / "llr.bin"), str(F), str(limit)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "fsscan gpu ok" in r.stdout
    chk = checker(oracle, 8)
    s, b, k, t = fsscan_decode(N, fr, llr, limit, chk)
    free = np.setdiff1d(np.arange(N), fr)
    for f, line in enumerate(r.stdout.splitlines()[:F]):
        okv, tr, info, soft, sinfo, ok2, info2, soft2 = line.split()
        assert (int(okv), int(tr)) == (int(k[f]), int(t[f])), f
        assert np.array_equal(np.frombuffer(bytes.fromhex(info), np.uint8), b[f]), f
        assert same_bits(np.frombuffer(bytes.fromhex(soft), np.float32), s[f]), f
        assert same_bits(np.frombuffer(bytes.fromhex(sinfo), np.float32), s[f][free]), f
        a = fsscan_decode(N, fr, llr[f:f + 1], int(t[f]) + 1, chk, forced=True)
        assert int(ok2) == int(a[2][0]), f
        assert np.array_equal(np.frombuffer(bytes.fromhex(info2), np.uint8), a[1][0]), f
        assert same_bits(np.frombuffer(bytes.fromhex(soft2), np.float32), a[0][0]), f


class Recording:
    """pcsim's GPU backend, keeping the frames it generated (as tests/test_gpu_pcsim.py)."""

    def __init__(self):
        from antpolarcodes_amd.pcsim import GpuBackend
        self.be = GpuBackend(0)
        self.llr, self.sent = [], []

    def setup(self, job):
        self.be.setup(job)

    def frames(self, job, F, seed):
        llr, info, t = self.be.frames(job, F, seed)
        self.llr.append(llr.cpu().numpy())
        self.sent.append(info.cpu().numpy())
        return llr, info, t

    def decode(self, job, llr):
        return self.be.decode(job, llr)

    def close(self):
        self.frozen = self.be.frozen
        self.kernel = self.be.plan.kernel_name()
        self.be.close()


@pytest.mark.parametrize("simtype", ["fastsscan", "scan"])
def test_pcsim_job_matches_restatement(oracle, simtype):
    """pcsim fastsscan / scan -n 256 -r 0.5 -e crc8 -p 32 --l-min 2 --l-max 2: the block, bit and
    reported error counts equal the restatements' decisions on the very same frames."""
    from antpolarcodes_amd import pcsim
    from scan_numpy import scan_decode
    a = pcsim.parser().parse_args([simtype, "-n", "256", "-r", "0.5", "-e", "crc8", "-p", "32", "--l-min", "2",
                                   "--l-max", "2", "-w", str(256 * 1000), "--snr-min", "1.0", "--snr-max", "2.0",
                                   "--snr-count", "4"])
    jobs = pcsim.build_jobs(a)
    assert [j.L for j in jobs] == [2] and jobs[0].decoder == simtype
    job, rec = jobs[0], Recording()
    pcsim.run_job(job, rec, batch=512, seed=5)
    assert rec.kernel == ("fsscan_kernel" if simtype == "fastsscan" else "scan_kernel")
    llr = np.concatenate(rec.llr[1:])  # the first call is the warm-up batch
    sent = np.concatenate(rec.sent[1:])
    assert llr.shape[0] == job.runs == 1000
    if simtype == "fastsscan":
        _, info, ok, _ = fsscan_decode(256, rec.frozen, llr, 2, checker(oracle, 8))
    else:
        info = scan_decode(256, rec.frozen, llr, 2, True)[2]
        ok = np.array([int(oracle.crc(8, row)) for row in info], np.uint8)
    be = np.unpackbits(np.bitwise_xor(sent, info), axis=1).sum(axis=1)
    assert job.errors == int((be > 0).sum())
    assert job.biterrors == int(be.sum())
    assert job.reportedErrors == int((ok == 0).sum())
    assert 0 < job.BLER < 1
