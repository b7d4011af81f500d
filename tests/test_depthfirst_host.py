"""The SC-Flip decoder without a GPU: host-only plans (pcg_plan_create_depthfirst with device < 0)
describe themselves and agree with the restatement's tree census, argument errors return their
codes, the other plans' entry points and this plan's refuse each other, pypolar.DepthFirstDecoder
and the C++ class PolarCode::Decoding::DepthFirst construct and validate, pcsim builds its
depthfirst job list, and decoding without a GPU fails loudly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits
from depthfirst_numpy import tree_census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "antpolarcodes_amd", "lib")


def _nat():
    from antpolarcodes_amd import _native
    return _native


@pytest.mark.parametrize("N,limit", [(8, 1), (16, 8), (1024, 8), (4096, 255)])
def test_host_only_plan_describes_itself(N, limit):
    nat = _nat()
    K = N // 2
    fr = frozen_bits(N, K, 0.0)
    c = tree_census(N, fr)
    for sysm in (True, False):
        p = nat.DepthFirstPlan(N, min(limit, K), fr, systematic=sysm, crc=8, device=-1)
        d = p.describe()
        assert d["block_length"] == N and d["info_length"] == K == c["info_leaves"]
        assert d["list_size"] == min(limit, K)  # the trial limit
        assert d["crc_kind"] == 8 and d["systematic"] == int(sysm)
        assert d["specialized"] == 0 and d["lanes_per_codeword"] == 0
        assert 0 < d["lds_bytes"] <= 160 * 1024
        # per codeword: the node inputs per level (2N words), the decoded words (N), the first
        # pass's reliabilities (K, padded to 4) and 256 search entries
        assert d["scratch_bytes"] == 4 * (3 * N + (K + 3) // 4 * 4 + 256)
        assert d["node_count"] == c["nodes"] and d["op_count"] == c["ops"]
        assert p.kernel_name() == "depthfirst_kernel"
        p.set_trials(2)
        assert p.describe()["list_size"] == 2


def test_schedule_census_of_16_8():
    """(16, 8): 31 nodes, 16 leaves of which 8 carry information; the plan walks the root's F, G
    and combine around two size-8 subtrees."""
    fr = frozen_bits(16, 8, 0.0)
    c = tree_census(16, fr)
    assert (c["nodes"], c["leaves"], c["info_leaves"], c["frozen_leaves"]) == (31, 16, 8, 8)
    assert (c["rater"], c["short_rater"], c["ops"]) == (1, 14, 5)
    d = _nat().DepthFirstPlan(16, 2, fr, device=-1).describe()
    assert (d["node_count"], d["op_count"], d["info_length"]) == (c["nodes"], c["ops"], c["info_leaves"])
    # any frozen set: nothing is pruned
    rng = np.random.default_rng(4)
    for _ in range(20):
        N = int(2 ** rng.integers(3, 9))
        K = int(rng.integers(2, N + 1))
        fr = sorted(rng.choice(N, N - K, replace=False).tolist())
        d = _nat().DepthFirstPlan(N, 2, fr, device=-1).describe()
        c = tree_census(N, fr)
        assert (d["node_count"], d["op_count"], d["info_length"]) == (c["nodes"], c["ops"], K)


def test_argument_errors():
    nat = _nat()
    fr = frozen_bits(64, 32, 0.0)

    def code(*a, **k):
        with pytest.raises(nat.PcgError) as e:
            nat.DepthFirstPlan(*a, device=-1, **k)
        return e.value.code

    assert code(48, 1, [0, 1]) == nat.PCG_E_ARG       # not a power of two
    assert code(4, 1, [0, 1]) == nat.PCG_E_ARG        # N < 8
    assert code(64, 1, [3, 2]) == nat.PCG_E_ARG       # unsorted
    assert code(64, 1, [1, 64]) == nat.PCG_E_ARG      # out of range
    assert code(64, 0, fr) == nat.PCG_E_ARG           # no trials
    assert code(64, 256, []) == nat.PCG_E_ARG         # trial limit > 255
    assert code(64, 33, fr) == nat.PCG_E_ARG          # K < T: the reference reads hintList[T - 1]
    assert code(8, 1, list(range(7))) == nat.PCG_E_ARG  # K = 1 < 2: the reference reads hintList[1]
    assert code(8, 1, list(range(8))) == nat.PCG_E_ARG  # K = 0
    assert code(64, 1, fr, crc=7) == nat.PCG_E_ARG    # no such detector
    assert code(8192, 1, frozen_bits(8192, 4096, 0.0)) == nat.PCG_E_UNSUPPORTED
    with pytest.raises(nat.PcgError, match="4096"):
        nat.DepthFirstPlan(8192, 1, frozen_bits(8192, 4096, 0.0), device=-1)
    nat.DepthFirstPlan(64, 32, fr, device=-1)         # K = T
    nat.DepthFirstPlan(8, 2, list(range(6)), device=-1)  # K = 2
    nat.DepthFirstPlan(256, 255, [0], device=-1)
    p = nat.DepthFirstPlan(64, 2, fr, device=-1)
    for bad in (0, 33, 256):
        with pytest.raises(nat.PcgError) as e:
            p.set_trials(bad)
        assert e.value.code == nat.PCG_E_ARG
    assert p.describe()["list_size"] == 2


def test_unsupported_entry_points_on_a_depthfirst_plan():
    nat = _nat()
    p = nat.DepthFirstPlan(64, 2, frozen_bits(64, 32, 0.0), device=-1)
    for wait in (True, False):
        with pytest.raises(nat.PcgError) as e:
            p.specialize(wait=wait)
        assert e.value.code == nat.PCG_E_UNSUPPORTED
    assert p.describe()["specialized"] == 0
    with pytest.raises(nat.PcgError) as e:
        p.decode_host_i8(np.zeros((2, 64), np.int8))
    assert e.value.code == nat.PCG_E_UNSUPPORTED
    L = nat.lib()
    z = np.zeros(64 * 2, np.int8)
    out = np.zeros(16, np.uint8)
    assert L.pcg_decode_i8(p._h, z.ctypes.data, 2, out.ctypes.data, None, None, None) == nat.PCG_E_UNSUPPORTED
    punc = nat.Puncturer(60, frozen_bits(64, 32, 0.0), device=-1)
    zf = np.zeros(64 * 2, np.float32)
    assert L.pcg_decode_punctured_f32(p._h, punc._h, zf.ctypes.data, 2, out.ctypes.data, None, None,
                                      None) == nat.PCG_E_UNSUPPORTED
    # the SCAN and Fast-SSCAN entry points refuse an SC-Flip plan
    assert L.pcg_decode_scan_f32_host(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None) == nat.PCG_E_ARG
    assert L.pcg_decode_scan_f32(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None, None) == nat.PCG_E_ARG
    assert L.pcg_plan_set_scan_iterations(p._h, 2) == nat.PCG_E_ARG
    assert L.pcg_decode_fsscan_f32_host(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None) == nat.PCG_E_ARG
    assert L.pcg_decode_fsscan_f32(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None, None) == nat.PCG_E_ARG
    assert L.pcg_plan_set_fsscan_trials(p._h, 2, 0) == nat.PCG_E_ARG


def test_depthfirst_decode_on_another_plan_is_an_argument_error():
    nat = _nat()
    L = nat.lib()
    fr = frozen_bits(64, 32, 0.0)
    z = np.zeros((2, 64), np.float32)
    out = np.zeros((2, 4), np.uint8)
    for p in (nat.Plan(64, 1, fr, device=-1), nat.ScanPlan(64, 1, fr, device=-1),
              nat.FastSscanPlan(64, 1, fr, device=-1)):
        assert L.pcg_decode_depthfirst_f32_host(p._h, z.ctypes.data, 2, out.ctypes.data, None, None, None) == \
            nat.PCG_E_ARG
        assert L.pcg_decode_depthfirst_f32(p._h, z.ctypes.data, 2, out.ctypes.data, None, None, None, None) == \
            nat.PCG_E_ARG
        assert L.pcg_plan_set_depthfirst_trials(p._h, 2) == nat.PCG_E_ARG


def test_host_only_plan_fails_loudly():
    nat = _nat()
    p = nat.DepthFirstPlan(64, 2, frozen_bits(64, 32, 0.0), device=-1)
    for call in (lambda: p.decode_host(np.zeros((2, 64), np.float32)),
                 lambda: nat.Plan.decode_host(p, np.zeros((2, 64), np.float32))):
        with pytest.raises(nat.PcgError) as e:
            call()
        assert e.value.code == nat.PCG_E_NODEVICE
    with pytest.raises(nat.PcgError) as e:  # no soft codeword on this plan
        p.decode_soft_host(np.zeros((2, 64), np.float32))
    assert e.value.code == nat.PCG_E_UNSUPPORTED


def test_pypolar_depthfirst_decoder_without_gpu():
    from antpolarcodes_amd import pypolar
    assert "DepthFirstDecoder" in pypolar.__all__
    fr = frozen_bits(256, 128, 0.0)
    dec = pypolar.DepthFirstDecoder(256, 4, fr)
    assert dec.blockLength() == 256 and dec.infoLength() == 128 and dec.listSize() == 4
    assert dec.isSystematic() and list(dec.frozenBits()) == list(fr) and dec.trials() == 0
    assert dec.getErrorDetectionMode() == "CRC-8"  # as makeDecoder would install
    dec.setTrialLimit(2)
    assert dec.listSize() == 2
    dec.setErrorDetection(32)
    assert dec.getErrorDetectionMode() == "CRC-32"
    dec.setSystematic(False)
    assert not dec.isSystematic()
    assert not hasattr(dec, "setErrorStatistics") and not hasattr(dec, "setNodeRanking")
    with pytest.raises(RuntimeError, match="Only ONE-dimensional vectors allowed!"):
        dec.decode_vector(np.zeros((2, 256), np.float32))
    with pytest.raises(RuntimeError, match="Input vector size != blockSize // 8!"):
        dec.decode_vector(np.zeros(255, np.float32))
    with pytest.raises(RuntimeError, match="decode_batch expects"):
        dec.decode_batch(np.zeros((2, 255), np.float32))
    for bad in (0, 129, 256):
        with pytest.raises(Exception):
            pypolar.DepthFirstDecoder(256, bad, fr)
        with pytest.raises(Exception):
            dec.setTrialLimit(bad)
    with pytest.raises(Exception):
        pypolar.DepthFirstDecoder(100, 2, [0, 1])


def test_pcsim_depthfirst_jobs():
    """configureDepthFirstSim (simulator.cpp:303-321): L = l-min, 2 l-min, ... <= l-max is the
    trial limit, with the decoder type set; float decoding only."""
    from antpolarcodes_amd import pcsim
    assert "depthfirst" in pcsim.SUPPORTED
    a = pcsim.parser().parse_args(["depthfirst", "-p", "32", "--l-min", "1", "--l-max", "8", "-n", "256"])
    jobs = pcsim.configure(a)
    assert [j.L for j in jobs] == [1, 2, 4, 8] and all(j.decoder == "depthfirst" and j.N == 256 for j in jobs)
    assert all(j.decoder == "depthfirst" for j in pcsim.build_jobs(a))
    for prec in ("8", "832"):
        with pytest.raises(SystemExit, match="32-bit"):
            pcsim.configure(pcsim.parser().parse_args(["depthfirst", "-p", prec]))
    with pytest.raises(SystemExit, match="32-bit"):
        pcsim.configure(pcsim.parser().parse_args(["depthfirst"]))  # the default precision is 832


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_depthfirst_class_through_the_reference_header(tmp_path):
    """tests/cpp/depthfirst_caller.cpp builds DepthFirst(1024, 8, frozen) through
    <polarcode/decoding/depth_first.h>."""
    exe = str(tmp_path / "depthfirst_caller")
    src = os.path.join(ROOT, "tests", "cpp", "depthfirst_caller.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", LIB, "-lpolarcode_amd", "-lpcg", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "api"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert "depthfirst api ok" in r.stdout
