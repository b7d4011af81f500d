"""The Fast-SSCAN decoder without a GPU: host-only plans (pcg_plan_create_fsscan with device < 0)
describe themselves and agree with the restatement's node census, argument errors return their
codes, pypolar.FastSscanDecoder and the C++ class PolarCode::Decoding::FastSscanFloat construct
and validate, pcsim builds its scan / fastsscan job lists, and decoding without a GPU fails
loudly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits
from fsscan_numpy import fsscan_census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "antpolarcodes_amd", "lib")


def _nat():
    from antpolarcodes_amd import _native
    return _native


@pytest.mark.parametrize("N,limit", [(8, 1), (1024, 4), (4096, 2)])
def test_host_only_plan_describes_itself(N, limit):
    nat = _nat()
    fr = frozen_bits(N, N // 2, 0.0)
    c = fsscan_census(N, fr)
    for sysm in (True, False):
        p = nat.FastSscanPlan(N, limit, fr, systematic=sysm, crc=8, device=-1)
        d = p.describe()
        assert d["block_length"] == N and d["info_length"] == N // 2
        assert d["list_size"] == limit  # the trial limit
        assert d["crc_kind"] == 8 and d["systematic"] == int(sysm)  # recorded, otherwise ignored
        assert d["specialized"] == 0 and d["lanes_per_codeword"] == 0
        assert 0 < d["lds_bytes"] <= 160 * 1024
        # per codeword: the inputs and the left children's messages per level (2N floats each),
        # and the messages of the non-constant right children
        assert d["scratch_bytes"] == 4 * (4 * N + c["right_floats"])
        assert d["node_count"] == c["nodes"] and d["op_count"] == c["ops"]
        assert p.kernel_name() == "fsscan_kernel"
        p.set_trials(7)
        assert p.describe()["list_size"] == 7
        p.set_trials(3, forced=True)
        assert p.describe()["list_size"] == 3


def test_any_frozen_set_and_its_census():
    """No Fast-SSC pattern restrictions; the plan's node and op counts equal the restatement's,
    the roots K = 0, 1, N - 1, N included."""
    nat = _nat()
    rng = np.random.default_rng(3)
    sets = [(8, []), (8, list(range(8))), (8, list(range(7))), (8, [0]), (16, list(range(15))), (16, [0])]
    for _ in range(60):
        N = int(2 ** rng.integers(3, 9))
        K = int(rng.integers(1, N))
        sets.append((N, sorted(rng.choice(N, N - K, replace=False).tolist())))
    right_twobit = 0
    for N, fr in sets:
        d = nat.FastSscanPlan(N, 2, fr, device=-1).describe()
        c = fsscan_census(N, fr)
        assert d["info_length"] == N - len(fr)
        assert (d["node_count"], d["op_count"], d["scratch_bytes"]) == \
            (c["nodes"], c["ops"], 4 * (4 * N + c["right_floats"])), (N, fr)
        right_twobit += c["right_twobit"] > 0
    assert right_twobit > 0


def test_argument_errors():
    nat = _nat()
    fr = frozen_bits(64, 32, 0.0)

    def code(*a, **k):
        with pytest.raises(nat.PcgError) as e:
            nat.FastSscanPlan(*a, device=-1, **k)
        return e.value.code

    assert code(48, 1, [0, 1]) == nat.PCG_E_ARG       # not a power of two
    assert code(4, 1, [0, 1]) == nat.PCG_E_ARG        # N < 8
    assert code(64, 1, [3, 2]) == nat.PCG_E_ARG       # unsorted
    assert code(64, 1, [2, 2]) == nat.PCG_E_ARG       # not strictly ascending
    assert code(64, 1, [1, 64]) == nat.PCG_E_ARG      # out of range
    assert code(64, 0, fr) == nat.PCG_E_ARG           # no passes: the reference returns stale output
    assert code(64, 256, fr) == nat.PCG_E_ARG         # trial limit > 255
    assert code(64, 1, fr, crc=7) == nat.PCG_E_ARG    # no such detector
    assert code(8192, 1, frozen_bits(8192, 4096, 0.0)) == nat.PCG_E_UNSUPPORTED
    with pytest.raises(nat.PcgError, match="4096"):
        nat.FastSscanPlan(8192, 1, frozen_bits(8192, 4096, 0.0), device=-1)
    nat.FastSscanPlan(64, 255, fr, device=-1)
    p = nat.FastSscanPlan(64, 2, fr, device=-1)
    for bad in (0, 256):
        with pytest.raises(nat.PcgError) as e:
            p.set_trials(bad)
        assert e.value.code == nat.PCG_E_ARG
    assert p.describe()["list_size"] == 2


def test_unsupported_entry_points_on_a_fsscan_plan():
    nat = _nat()
    p = nat.FastSscanPlan(64, 2, frozen_bits(64, 32, 0.0), device=-1)
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
    # the SCAN entry points refuse a Fast-SSCAN plan
    assert L.pcg_decode_scan_f32_host(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None) == nat.PCG_E_ARG
    assert L.pcg_decode_scan_f32(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None, None) == nat.PCG_E_ARG
    assert L.pcg_plan_set_scan_iterations(p._h, 2) == nat.PCG_E_ARG


def test_fsscan_decode_on_another_plan_is_an_argument_error():
    nat = _nat()
    L = nat.lib()
    fr = frozen_bits(64, 32, 0.0)
    z = np.zeros((2, 64), np.float32)
    out = np.zeros((2, 4), np.uint8)
    for p in (nat.Plan(64, 1, fr, device=-1), nat.ScanPlan(64, 1, fr, device=-1)):
        assert L.pcg_decode_fsscan_f32_host(p._h, z.ctypes.data, 2, out.ctypes.data, None, None, None) == nat.PCG_E_ARG
        assert L.pcg_decode_fsscan_f32(p._h, z.ctypes.data, 2, out.ctypes.data, None, None, None, None) == \
            nat.PCG_E_ARG
        assert L.pcg_plan_set_fsscan_trials(p._h, 2, 0) == nat.PCG_E_ARG


def test_host_only_plan_fails_loudly():
    nat = _nat()
    p = nat.FastSscanPlan(64, 2, frozen_bits(64, 32, 0.0), device=-1)
    for call in (lambda: p.decode_host(np.zeros((2, 64), np.float32)),
                 lambda: nat.Plan.decode_host(p, np.zeros((2, 64), np.float32)),
                 lambda: p.decode_soft_host(np.zeros((2, 64), np.float32))):
        with pytest.raises(nat.PcgError) as e:
            call()
        assert e.value.code == nat.PCG_E_NODEVICE


def test_pypolar_fastsscan_decoder_without_gpu():
    from antpolarcodes_amd import pypolar
    assert "FastSscanDecoder" in pypolar.__all__
    fr = frozen_bits(256, 128, 0.0)
    dec = pypolar.FastSscanDecoder(256, 4, fr)
    assert dec.blockLength() == 256 and dec.infoLength() == 128 and dec.listSize() == 4
    assert dec.isSystematic() and list(dec.frozenBits()) == list(fr)
    assert dec.getErrorDetectionMode() == "CRC-8"  # as makeDecoder would install
    dec.setTrialLimit(2)
    assert dec.listSize() == 2
    dec.setErrorDetection(16)
    assert dec.getErrorDetectionMode() == "CRC-16"
    dec.setSystematic(False)  # accepted and without effect, as in the reference
    assert not dec.isSystematic()
    with pytest.raises(RuntimeError, match="Only ONE-dimensional vectors allowed!"):
        dec.decode_vector(np.zeros((2, 256), np.float32))
    with pytest.raises(RuntimeError, match="Input vector size != blockSize // 8!"):
        dec.decode_vector(np.zeros(255, np.float32))
    with pytest.raises(RuntimeError, match="decode_batch expects"):
        dec.decode_batch(np.zeros((2, 255), np.float32))
    with pytest.raises(Exception, match="decode"):
        dec.decodeAgain()  # nothing decoded yet
    for bad in (0, 256):
        with pytest.raises(Exception):
            pypolar.FastSscanDecoder(256, bad, fr)
    with pytest.raises(Exception):
        pypolar.FastSscanDecoder(100, 2, [0, 1])


def test_pcsim_scan_and_fastsscan_jobs():
    """configureScanSim (simulator.cpp:323-340): L = l-min, 2 l-min, ... <= l-max with the decoder
    type set; float decoding only."""
    from antpolarcodes_amd import pcsim
    assert {"scan", "fastsscan"} <= set(pcsim.SUPPORTED)
    for st in ("scan", "fastsscan"):
        a = pcsim.parser().parse_args([st, "-p", "32", "--l-min", "1", "--l-max", "8", "-n", "256"])
        jobs = pcsim.configure(a)
        assert [j.L for j in jobs] == [1, 2, 4, 8] and all(j.decoder == st and j.N == 256 for j in jobs)
        assert all(j.decoder == st for j in pcsim.build_jobs(a))
        for prec in ("8", "832"):
            with pytest.raises(SystemExit, match="32-bit"):
                pcsim.configure(pcsim.parser().parse_args([st, "-p", prec]))
    # the other simulation types keep the flexible decoder
    assert all(j.decoder == "" for j in pcsim.configure(pcsim.parser().parse_args(["listlength"])))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_fastsscan_class_through_the_reference_header(tmp_path):
    """tests/cpp/fsscan_caller.cpp builds FastSscanFloat(1024, 4, frozen) through
    <polarcode/decoding/fastsscan_float.h>."""
    exe = str(tmp_path / "fsscan_caller")
    src = os.path.join(ROOT, "tests", "cpp", "fsscan_caller.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", LIB, "-lpolarcode_amd", "-lpcg", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "api"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert "fsscan api ok" in r.stdout
