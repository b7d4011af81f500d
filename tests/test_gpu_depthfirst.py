"""The SC-Flip kernel (depthfirst_kernel.hip) on the GPU, byte for byte against the reference's
recorded outputs (tests/golden/depthfirst_fixtures.npz) and, where there is no fixture or the
search meets ties, against tests/depthfirst_numpy.py under the stable tie rule (pinned to the same
fixtures by tests/test_depthfirst_restatement.py).  The decoded codeword is compared as 32-bit
words."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits
from depthfirst_numpy import depthfirst_decode
from helpers import LLR_KINDS, llr_kinds
from test_depthfirst_restatement import checker, fixture_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "antpolarcodes_amd", "lib")
GOLD = os.path.join(ROOT, "tests", "golden", "depthfirst_fixtures.npz")


def _nat():
    from antpolarcodes_amd import _native
    return _native


def check(got, want, tag, K=None):
    """got = (info, ok, bits, trials) of the plan, want = (bits, info, ok, trials) of the checker."""
    info, ok, bits, trials = got
    w, b, k, t = want[:4]
    assert np.array_equal(trials, t), (tag, "trials", trials.tolist(), np.asarray(t).tolist())
    assert np.array_equal(ok, k), (tag, "ok")
    assert bits.dtype == np.uint32 and np.array_equal(bits, w), (tag, "bits")
    if K is not None and K % 8:
        assert np.array_equal(np.unpackbits(info, axis=1)[:, :K], np.unpackbits(b, axis=1)[:, :K]), (tag, "info")
    else:
        assert np.array_equal(info, b), (tag, "info")


def test_reference_fixtures():
    """Every recorded case: N = 8 (ShortRateR nodes only), 16 (one RateR over them), 32, 64, 256
    and 1024; limits 1 (all LLR kinds: plain SC, one trial everywhere), 2, 3, 4, 8, 32; the dummy
    detector, CRC-8, CRC-32; non-systematic; random frozen sets."""
    nat = _nat()
    seen, n = set(), 0
    for i, N, fr, limit, crc, sysm, llr, bits, info, ok, trials, depth in fixture_cases():
        p = nat.DepthFirstPlan(N, limit, fr, systematic=sysm, crc=crc)
        assert p.kernel_name() == "depthfirst_kernel"
        check(p.decode_host(llr), (bits, info, ok, trials), (i, N, limit, crc, sysm), N - len(fr))
        if limit == 1 or crc == 0:
            assert (trials == 1).all()
        p.close()
        seen.add((N, limit, crc, sysm))
        n += 1
    assert n >= 40
    assert {8, 16, 32, 64, 256, 1024} <= {s[0] for s in seen} and {0, 8, 32} <= {s[2] for s in seen}
    assert any(not s[3] for s in seen)


def test_one_wave_mixes_every_outcome_of_the_search():
    """The limit-32 fixture case in one wave: lanes that pass at trial 1, at a depth-0 flip, at a
    depth-1 configuration, and lanes that never pass.  A lane that passed early keeps its own
    outputs and its own trial count -- also when its neighbours' outputs are not asked for."""
    nat = _nat()
    i = int(np.load(GOLD)["mix_case"][0])
    _, N, fr, limit, crc, sysm, llr, bits, info, ok, trials, depth = list(fixture_cases())[i]
    assert limit == 32 and llr.shape[0] <= 64
    assert (trials == 1).any() and ((ok == 1) & (trials > 1) & (depth == 0)).any()
    assert ((ok == 1) & (depth == 1)).any() and ((ok == 0) & (trials == 32) & (depth == 1)).any()
    p = nat.DepthFirstPlan(N, limit, fr, crc=crc)
    check(p.decode_host(llr), (bits, info, ok, trials), "mix")
    i2, k2, b2, t2 = p.decode_host(llr, want_bits=False)
    assert b2 is None and np.array_equal(i2, info) and np.array_equal(k2, ok) and np.array_equal(t2, trials)
    i3, k3, b3, t3 = p.decode_host(llr, want_ok=False, want_trials=False)
    assert k3 is None and t3 is None and np.array_equal(i3, info) and np.array_equal(b3, bits)
    # the same lanes in another order and spread over two waves
    perm = np.random.default_rng(1).permutation(np.tile(np.arange(llr.shape[0]), 5))
    check(p.decode_host(llr[perm]), (bits[perm], info[perm], ok[perm], trials[perm]), "mix, two waves")


@pytest.mark.parametrize("N,K,T", [(8, 4, 3), (16, 8, 8), (64, 32, 8), (256, 128, 4), (4096, 2048, 2)])
def test_shape_edges(oracle, N, K, T):
    """F = 1, 63, 65, 130: partial waves and more than one wave, AWGN frames through CRC-8 so that
    lanes stop at different trials."""
    from antpolarcodes_amd import frames
    nat = _nat()
    fr = frozen_bits(N, K, 0.0)
    Fmax = 130 if N <= 256 else 65
    llr = frames.awgn_frames(N, fr, Fmax, 1.5, seed=N, crc=8 if K > 8 else 0)[0]
    crc = 8 if K > 8 else 0
    if crc:
        want = depthfirst_decode(N, fr, llr, T, checker(oracle, crc))
        assert not want[4].any()
        if N <= 256:
            assert want[3].min() == 1 and want[3].max() == T
        p = nat.DepthFirstPlan(N, T, fr, crc=crc)
        for F in (1, 63, 65, 130):
            if F <= Fmax:
                check(p.decode_host(llr[:F]), tuple(w[:F] for w in want), (N, K, T, F), K)
    else:  # too few information bits for a CRC: the dummy detector, one trial
        want = depthfirst_decode(N, fr, llr, T, None)
        p = nat.DepthFirstPlan(N, T, fr, crc=0)
        for F in (1, 63, 65, 130):
            check(p.decode_host(llr[:F]), tuple(w[:F] for w in want), (N, K, T, F), K)
        assert (want[3] == 1).all()


@pytest.mark.parametrize("T", [2, 8])
def test_tie_heavy_kinds_follow_the_stable_rule(oracle, T):
    """"ints", "sparse", "zeros": equal reliabilities everywhere.  The kernel equals the
    restatement with ties to the lower leaf index (not the reference, whose order among equals is
    std::sort's)."""
    nat = _nat()
    rng = np.random.default_rng(20 + T)
    ambiguous = 0
    for N, K in ((64, 32), (256, 100)):
        fr = frozen_bits(N, K, 0.0)
        llr = np.concatenate([llr_kinds(rng, 22, N, k) for k in ("ints", "sparse", "zeros")])
        for sysm in (True, False):
            want = depthfirst_decode(N, fr, llr, T, checker(oracle, 8), sysm)
            ambiguous += int(want[4].sum())
            assert want[3].max() == T
            p = nat.DepthFirstPlan(N, T, fr, systematic=sysm, crc=8)
            check(p.decode_host(llr), want, (N, K, T, sysm), K)
    assert ambiguous > 40


def test_limit_one_is_plain_sc(oracle):
    nat = _nat()
    rng = np.random.default_rng(3)
    N, fr = 128, frozen_bits(128, 64, 0.0)
    llr = np.concatenate([llr_kinds(rng, 14, N, k) for k in LLR_KINDS])
    for crc in (0, 8):
        want = depthfirst_decode(N, fr, llr, 1, checker(oracle, crc))
        assert (want[3] == 1).all()
        check(nat.DepthFirstPlan(N, 1, fr, crc=crc).decode_host(llr), want, crc)
    # the dummy detector stops every frame after trial 1 whatever the limit
    check(nat.DepthFirstPlan(N, 9, fr, crc=0).decode_host(llr), want[:2] + (np.ones(70, np.uint8), want[3]), "dummy")


@pytest.mark.parametrize("N", [32, 64])
def test_random_frozen_sets(oracle, N):
    nat = _nat()
    rng = np.random.default_rng(500 + N)
    for _ in range(12):
        K = int(rng.integers(9, N))
        fr = sorted(rng.choice(N, N - K, replace=False).tolist())
        llr = np.concatenate([llr_kinds(rng, 5, N, "normal"), llr_kinds(rng, 3, N, "wide")])
        T = int(rng.integers(1, min(K, 12) + 1))
        sysm = bool(rng.integers(0, 2))
        want = depthfirst_decode(N, fr, llr, T, checker(oracle, 8), sysm)
        p = nat.DepthFirstPlan(N, T, fr, systematic=sysm, crc=8)
        check(p.decode_host(llr), want, (N, fr, T, sysm), K)
        p.close()


def test_set_trials_between_decodes(oracle):
    from antpolarcodes_amd import frames
    nat = _nat()
    N, fr = 64, frozen_bits(64, 32, 0.0)
    llr = frames.awgn_frames(N, fr, 70, 1.0, seed=9, crc=8)[0]
    p = nat.DepthFirstPlan(N, 1, fr, crc=8)
    for T in (1, 8, 2, 32, 1):
        p.set_trials(T)
        assert p.describe()["list_size"] == T
        want = depthfirst_decode(N, fr, llr, T, checker(oracle, 8))
        check(p.decode_host(llr), want, T)
    a = p.decode_host(llr)
    p.decode_host(llr * np.float32(-1.0))
    for x, y in zip(a, p.decode_host(llr)):  # no state is carried between calls
        assert np.array_equal(x, y)


def test_device_path_streams_and_untouched_outputs(oracle):
    import itertools
    import torch
    from antpolarcodes_amd import frames
    nat = _nat()
    N, fr, F, T = 256, frozen_bits(256, 128, 0.0), 130, 4
    llr = frames.awgn_frames(N, fr, F, 1.0, seed=4, crc=8)[0]
    w, b, k, t, amb = depthfirst_decode(N, fr, llr, T, checker(oracle, 8))
    assert not amb.any() and len(set(t.tolist())) >= 3
    p = nat.DepthFirstPlan(N, T, fr, crc=8)
    host = p.decode_host(llr)
    check(host, (w, b, k, t), "host")
    dev = torch.device("cuda:0")
    x = torch.from_numpy(llr).to(dev)
    stream = torch.cuda.Stream(device=dev)
    for want_ok, want_bits, want_trials in itertools.product((True, False), repeat=3):
        info = torch.full((F, p.kb), 0xAA, dtype=torch.uint8, device=dev)
        ok = torch.full((F,), 7, dtype=torch.uint8, device=dev)
        trials = torch.full((F,), 77, dtype=torch.uint8, device=dev)
        bits = torch.full((F, N), 12345, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            p.decode_device(x, info, ok if want_ok else None, bits if want_bits else None,
                            trials if want_trials else None, stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(info.cpu().numpy(), host[0])  # the same bytes as the host-pointer decode
        assert np.array_equal(ok.cpu().numpy(), k) if want_ok else (ok.cpu().numpy() == 7).all()
        assert np.array_equal(trials.cpu().numpy(), t) if want_trials else (trials.cpu().numpy() == 77).all()
        got = bits.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, w) if want_bits else (got == 12345).all()
    # frames that start 4 bytes into an allocation: the kernel's other way of reading them
    y = torch.zeros(F * N + 1, dtype=torch.float32, device=dev)[1:].view(F, N)
    y.copy_(x)
    assert y.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    info = torch.zeros((F, p.kb), dtype=torch.uint8, device=dev)
    ok = torch.zeros((F,), dtype=torch.uint8, device=dev)
    bits = torch.zeros((F, N), dtype=torch.int32, device=dev)
    trials = torch.zeros((F,), dtype=torch.uint8, device=dev)
    p.decode_device(y, info, ok, bits, trials)
    torch.cuda.synchronize()
    check((info.cpu().numpy(), ok.cpu().numpy(), bits.cpu().numpy().view(np.uint32), trials.cpu().numpy()),
          (w, b, k, t), "offset")
    # the generic entry points: info and ok
    info.zero_(), ok.zero_()
    nat.Plan.decode_device(p, x, info, ok)
    torch.cuda.synchronize()
    assert np.array_equal(info.cpu().numpy(), b) and np.array_equal(ok.cpu().numpy(), k)
    i2, k2 = nat.Plan.decode_host(p, llr)[:2]
    assert np.array_equal(i2, b) and np.array_equal(k2, k)


def test_host_path_across_a_chunk_boundary():
    """pcg_decode_depthfirst_f32_host goes through the chunking helper SCAN and Fast-SSCAN share:
    N = 8 has the 65536-frame chunk; one frame more makes a second chunk."""
    nat = _nat()
    N, fr, F = 8, [0, 1, 2, 4], 65536 + 1
    llr = np.random.default_rng(2).normal(0, 2, (F, N)).astype(np.float32)
    p = nat.DepthFirstPlan(N, 3, fr, crc=0)
    check(p.decode_host(llr), depthfirst_decode(N, fr, llr, 3), "chunk + 1", 4)


def test_pypolar_decoder(oracle):
    from antpolarcodes_amd import frames, pypolar
    N, fr, T = 256, frozen_bits(256, 128, 0.0), 8
    llr = frames.awgn_frames(N, fr, 8, 0.5, seed=3, crc=8)[0]
    w, b, k, t, _ = depthfirst_decode(N, fr, llr, T, checker(oracle, 8))
    assert t.max() > 1
    dec = pypolar.DepthFirstDecoder(N, T, fr)
    info, ok, bits, trials = dec.decode_batch(llr, return_ok=True, return_bits=True, return_trials=True)
    check((info, ok, bits, trials), (w, b, k, t), "decode_batch")
    assert np.array_equal(dec.decode_batch(llr), b)
    for f in range(8):
        assert np.array_equal(dec.decode_vector(llr[f]), b[f])
        assert dec.trials() == t[f]
        assert np.array_equal(dec.getSoftCodeword().view(np.uint32), w[f])
    dec.setSystematic(False)
    dec.setTrialLimit(3)
    ns = depthfirst_decode(N, fr, llr, 3, checker(oracle, 8), systematic=False)
    check(dec.decode_batch(llr, return_ok=True, return_bits=True, return_trials=True), ns, "non-systematic")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_single_frame_flow(tmp_path, oracle):
    """setSignal -> decode -> getDecodedInformationBits -> getSoftCodeword of
    PolarCode::Decoding::DepthFirst, then decodeBatchBits (tests/cpp/depthfirst_caller.cpp)."""
    from antpolarcodes_amd import frames
    exe = str(tmp_path / "depthfirst_caller")
    src = os.path.join(ROOT, "tests", "cpp", "depthfirst_caller.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", LIB, "-lpolarcode_amd", "-lpcg", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    N, F, limit = 1024, 4, 8
    fr = frozen_bits(N, 512, 0.0)
    llr = frames.awgn_frames(N, fr, F, 1.5, seed=5, crc=8)[0]
    (tmp_path / "frozen.txt").write_text(" ".join(str(v) for v in fr))
    (tmp_path / "llr.bin").write_bytes(np.ascontiguousarray(llr, np.float32).tobytes())
    r = subprocess.run([exe, "gpu", str(tmp_path / "frozen.txt"), str(tmp_path / "llr.bin"), str(F), str(N),
                        str(limit), "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "depthfirst gpu ok" in r.stdout
    w, b, k, t, _ = depthfirst_decode(N, fr, llr, limit, checker(oracle, 8))
    lines = r.stdout.splitlines()
    for f, line in enumerate(lines[:F]):
        okv, tr, info, words = line.split()
        assert (int(okv), int(tr)) == (int(k[f]), int(t[f])), f
        assert np.array_equal(np.frombuffer(bytes.fromhex(info), np.uint8), b[f]), f
        assert np.array_equal(np.frombuffer(bytes.fromhex(words), np.uint32), w[f]), f
    binfo, bok, btr, bbits = (bytes.fromhex(v) for v in lines[F].split())
    assert np.array_equal(np.frombuffer(binfo, np.uint8).reshape(F, -1), b)
    assert np.array_equal(np.frombuffer(bok, np.uint8), k) and np.array_equal(np.frombuffer(btr, np.uint8), t)
    assert np.array_equal(np.frombuffer(bbits, np.uint32).reshape(F, N), w)


def test_pcsim_depthfirst_run(oracle):
    """pcsim depthfirst -p 32 -n 256 --l-min 1 --l-max 4 on one seed: the counts equal the
    restatement's decisions on the very same frames, and more trials never add frame errors (a
    frame whose first decode passes its check is final at every limit; the others were errors)."""
    from antpolarcodes_amd import pcsim
    from test_gpu_fsscan import Recording
    a = pcsim.parser().parse_args(["depthfirst", "-n", "256", "-r", "0.5", "-e", "crc8", "-p", "32", "--l-min", "1",
                                   "--l-max", "4", "-w", str(256 * 600), "--snr-min", "1.0", "--snr-max", "2.0",
                                   "--snr-count", "4"])
    jobs = pcsim.build_jobs(a)
    assert [j.L for j in jobs] == [1, 2, 4] and all(j.decoder == "depthfirst" for j in jobs)
    done = {}
    for job in (jobs[0], jobs[2]):
        rec = Recording()
        pcsim.run_job(job, rec, batch=512, seed=5)
        assert rec.kernel == "depthfirst_kernel"
        llr, sent = np.concatenate(rec.llr[1:]), np.concatenate(rec.sent[1:])  # the first call is the warm-up
        assert llr.shape[0] == job.runs == 600
        _, info, ok, _, amb = depthfirst_decode(256, rec.frozen, llr, job.L, checker(oracle, 8))
        assert not amb.any()
        be = np.unpackbits(np.bitwise_xor(sent, info), axis=1).sum(axis=1)
        assert job.errors == int((be > 0).sum()) and job.biterrors == int(be.sum())
        assert job.reportedErrors == int((ok == 0).sum())
        done[job.L] = (job, llr)
    assert np.array_equal(done[1][1], done[4][1])  # the same frames
    assert 0 < done[4][0].errors <= done[1][0].errors
    assert done[4][0].reportedErrors < done[1][0].reportedErrors
