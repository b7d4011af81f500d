"""The SCAN decoder without a GPU: host-only plans (pcg_plan_create_scan with device < 0)
describe themselves, argument errors return their codes, pypolar.ScanDecoder and the C++ class
PolarCode::Decoding::Scan construct and validate, and decoding without a GPU fails loudly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "antpolarcodes_amd", "lib")


def _nat():
    from antpolarcodes_amd import _native
    return _native


@pytest.mark.parametrize("N,it", [(8, 1), (1024, 4), (4096, 2)])
def test_host_only_plan_describes_itself(N, it):
    nat = _nat()
    for sysm in (True, False):
        p = nat.ScanPlan(N, it, frozen_bits(N, N // 2, 0.0), systematic=sysm, crc=8, device=-1)
        d = p.describe()
        assert d["block_length"] == N and d["info_length"] == N // 2
        assert d["list_size"] == it  # Scan::getListSize returns the iteration limit
        assert d["crc_kind"] == 8 and d["systematic"] == int(sysm)
        assert d["specialized"] == 0 and d["lanes_per_codeword"] == 0
        assert 0 < d["lds_bytes"] <= 160 * 1024
        # per codeword: L and E (2N floats each), O ((log2 N - 1) N/2), non-systematic: + N outputs
        n = N.bit_length() - 1
        assert d["scratch_bytes"] == 4 * (4 * N + (n - 1) * N // 2 + (0 if sysm else N))
        assert d["op_count"] > 0
        assert p.kernel_name() == "scan_kernel"
        p.set_iterations(7)
        assert p.describe()["list_size"] == 7


def test_any_frozen_set_is_accepted():
    """SCAN has no Fast-SSC pattern restrictions: sets the Fast-SSC plan refuses build here."""
    nat = _nat()
    rng = np.random.default_rng(3)
    refused = 0
    for _ in range(60):
        N = int(2 ** rng.integers(3, 9))
        K = int(rng.integers(1, N))
        fr = sorted(rng.choice(N, N - K, replace=False).tolist())
        assert nat.ScanPlan(N, 2, fr, device=-1).describe()["info_length"] == K
        try:
            nat.Plan(N, 1, fr, device=-1)
        except nat.PcgError as e:
            refused += e.code == nat.PCG_E_FROZEN
    assert refused > 0


def test_argument_errors():
    nat = _nat()
    fr = frozen_bits(64, 32, 0.0)

    def code(*a, **k):
        with pytest.raises(nat.PcgError) as e:
            nat.ScanPlan(*a, device=-1, **k)
        return e.value.code

    assert code(48, 1, [0, 1]) == nat.PCG_E_ARG       # not a power of two
    assert code(4, 1, [0, 1]) == nat.PCG_E_ARG        # N < 8
    assert code(64, 1, [3, 2]) == nat.PCG_E_ARG       # unsorted
    assert code(64, 1, [2, 2]) == nat.PCG_E_ARG       # not strictly ascending
    assert code(64, 1, [1, 64]) == nat.PCG_E_ARG      # out of range
    assert code(64, 256, fr) == nat.PCG_E_ARG         # iterations > 255
    assert code(64, 1, fr, crc=7) == nat.PCG_E_ARG    # no such detector
    assert code(8192, 1, frozen_bits(8192, 4096, 0.0)) == nat.PCG_E_UNSUPPORTED
    with pytest.raises(nat.PcgError, match="4096"):
        nat.ScanPlan(8192, 1, frozen_bits(8192, 4096, 0.0), device=-1)
    nat.ScanPlan(64, 255, fr, device=-1)
    nat.ScanPlan(64, 0, fr, device=-1)
    p = nat.ScanPlan(64, 2, fr, device=-1)
    with pytest.raises(nat.PcgError) as e:
        p.set_iterations(256)
    assert e.value.code == nat.PCG_E_ARG


def test_unsupported_entry_points_on_a_scan_plan():
    nat = _nat()
    p = nat.ScanPlan(64, 2, frozen_bits(64, 32, 0.0), device=-1)
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
    zf = np.zeros(60 * 2, np.float32)
    assert L.pcg_decode_punctured_f32(p._h, punc._h, zf.ctypes.data, 2, out.ctypes.data, None, None,
                                      None) == nat.PCG_E_UNSUPPORTED


def test_scan_decode_on_another_plan_is_an_argument_error():
    nat = _nat()
    L = nat.lib()
    p = nat.Plan(64, 1, frozen_bits(64, 32, 0.0), device=-1)
    z = np.zeros((2, 64), np.float32)
    out = np.zeros((2, 4), np.uint8)
    assert L.pcg_decode_scan_f32_host(p._h, z.ctypes.data, 2, out.ctypes.data, None, None, None) == nat.PCG_E_ARG
    assert L.pcg_decode_scan_f32(p._h, z.ctypes.data, 2, out.ctypes.data, None, None, None, None) == nat.PCG_E_ARG
    assert L.pcg_plan_set_scan_iterations(p._h, 2) == nat.PCG_E_ARG


def test_host_only_plan_fails_loudly():
    nat = _nat()
    p = nat.ScanPlan(64, 2, frozen_bits(64, 32, 0.0), device=-1)
    for call in (lambda: p.decode_host(np.zeros((2, 64), np.float32)),
                 lambda: nat.Plan.decode_host(p, np.zeros((2, 64), np.float32)),
                 lambda: p.decode_soft_host(np.zeros((2, 64), np.float32))):
        with pytest.raises(nat.PcgError) as e:
            call()
        assert e.value.code == nat.PCG_E_NODEVICE


def test_pypolar_scan_decoder_without_gpu():
    from antpolarcodes_amd import pypolar
    assert "ScanDecoder" in pypolar.__all__
    fr = frozen_bits(256, 128, 0.0)
    dec = pypolar.ScanDecoder(256, 4, fr)
    assert dec.blockLength() == 256 and dec.infoLength() == 128 and dec.listSize() == 4
    assert dec.isSystematic() and list(dec.frozenBits()) == list(fr)
    assert dec.getErrorDetectionMode() == "CRC-8"  # as makeDecoder would install
    dec.setIterationLimit(2)
    assert dec.listSize() == 2
    dec.setErrorDetection(16)
    assert dec.getErrorDetectionMode() == "CRC-16"
    dec.setSystematic(False)
    assert not dec.isSystematic()
    # PolarDecoder's error strings
    with pytest.raises(RuntimeError, match="Only ONE-dimensional vectors allowed!"):
        dec.decode_vector(np.zeros((2, 256), np.float32))
    with pytest.raises(RuntimeError, match="Input vector size != blockSize // 8!"):
        dec.decode_vector(np.zeros(255, np.float32))
    with pytest.raises(RuntimeError, match="decode_batch expects"):
        dec.decode_batch(np.zeros((2, 255), np.float32))
    with pytest.raises(Exception):
        pypolar.ScanDecoder(256, 256, fr)
    with pytest.raises(Exception):
        pypolar.ScanDecoder(100, 2, [0, 1])
    # the string route still refuses (a follow-up routes it to this class)
    with pytest.raises(Exception, match="not part of this build"):
        pypolar.PolarDecoder(256, 4, fr, "scan")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_scan_class_through_the_reference_header(tmp_path):
    """tests/cpp/scan_caller.cpp builds Scan(1024, 4, frozen) through <polarcode/decoding/scan.h>."""
    exe = str(tmp_path / "scan_caller")
    src = os.path.join(ROOT, "tests", "cpp", "scan_caller.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", LIB, "-lpolarcode_amd", "-lpcg", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "api"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert "scan api ok" in r.stdout
