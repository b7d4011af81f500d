"""The error locator without a GPU: host-only plans (pcg_plan_create_errorlocator with device < 0)
describe themselves, argument errors return their codes, the other plans' entry points and this
plan's refuse each other, pypolar.ErrorLocator and the C++ class PolarCode::Decoding::ErrorLocator
construct and validate, decoding without a GPU fails loudly, and the errorlocator tool parses its
options, builds its job, counts and writes its CSV with a mocked backend."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from antpolarcodes_amd.construction import frozen_bits
from test_errorlocator_restatement import gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "antpolarcodes_amd", "lib")


def _nat():
    from antpolarcodes_amd import _native
    return _native


@pytest.mark.parametrize("N", [8, 16, 1024, 4096])
def test_host_only_plan_describes_itself(N):
    nat = _nat()
    K = N // 2
    fr = frozen_bits(N, K, 0.0)
    p = nat.ErrorLocatorPlan(N, fr, device=-1)
    d = p.describe()
    flip = nat.DepthFirstPlan(N, 1, fr, device=-1).describe()
    assert d["block_length"] == N and d["info_length"] == K
    assert d["crc_kind"] == 0 and d["specialized"] == 0 and d["lanes_per_codeword"] == 0
    assert 0 < d["lds_bytes"] <= 160 * 1024
    # per codeword: the node inputs per level (2N words), the decoded words (N), the desired /
    # leaf values (N)
    assert d["scratch_bytes"] == 4 * 4 * N
    assert (d["node_count"], d["op_count"]) == (flip["node_count"], flip["op_count"])
    assert d["node_count"] == 2 * N - 1 and d["op_count"] == N // 8 + 3 * (N // 8 - 1)
    assert p.kernel_name() == "errorlocator_kernel"


def test_argument_errors():
    nat = _nat()

    def code(*a):
        with pytest.raises(nat.PcgError) as e:
            nat.ErrorLocatorPlan(*a, device=-1)
        return e.value.code

    assert code(48, [0, 1]) == nat.PCG_E_ARG            # not a power of two
    assert code(4, [0, 1]) == nat.PCG_E_ARG             # N < 8
    assert code(64, [3, 2]) == nat.PCG_E_ARG            # unsorted
    assert code(64, [2, 2]) == nat.PCG_E_ARG            # not strictly ascending
    assert code(64, [1, 64]) == nat.PCG_E_ARG           # out of range
    assert code(8, list(range(8))) == nat.PCG_E_ARG     # no information bit
    assert code(8192, frozen_bits(8192, 4096, 0.0)) == nat.PCG_E_UNSUPPORTED
    with pytest.raises(nat.PcgError, match="4096"):
        nat.ErrorLocatorPlan(8192, [0], device=-1)
    nat.ErrorLocatorPlan(8, list(range(7)), device=-1)  # K = 1: no trial-limit rule here
    nat.ErrorLocatorPlan(4096, [], device=-1)           # K = N
    L = nat.lib()
    p = nat.ErrorLocatorPlan(64, frozen_bits(64, 32, 0.0), device=-1)
    z = np.zeros((2, 64), np.float32)
    first = np.zeros(2, np.int32)
    for mode in (-1, 3, 99):  # unknown modes
        assert L.pcg_errorlocator_f32_host(p._h, mode, z.ctypes.data, None, 2, None, None, first.ctypes.data,
                                           None) == nat.PCG_E_ARG
        assert L.pcg_errorlocator_f32(p._h, mode, z.ctypes.data, None, 2, None, None, first.ctypes.data, None,
                                      None) == nat.PCG_E_ARG
    assert L.pcg_errorlocator_f32_host(p._h, 1, None, None, 2, None, None, first.ctypes.data, None) == nat.PCG_E_ARG
    assert L.pcg_errorlocator_f32(p._h, 1, None, None, 2, None, None, first.ctypes.data, None, None) == nat.PCG_E_ARG
    assert L.pcg_errorlocator_f32_host(None, 1, z.ctypes.data, None, 2, None, None, None, None) == nat.PCG_E_ARG
    with pytest.raises(ValueError):
        p.locate_host(z, mode="genie")
    with pytest.raises(ValueError):
        p.locate_host(z, desired=np.zeros((3, 64), np.float32))


def test_unsupported_entry_points_on_an_error_locator_plan():
    nat = _nat()
    fr = frozen_bits(64, 32, 0.0)
    p = nat.ErrorLocatorPlan(64, fr, device=-1)
    U, A = nat.PCG_E_UNSUPPORTED, nat.PCG_E_ARG
    for wait in (True, False):
        with pytest.raises(nat.PcgError) as e:
            p.specialize(wait=wait)
        assert e.value.code == U
    L = nat.lib()
    z8 = np.zeros(64 * 2, np.int8)
    zf = np.zeros(64 * 2, np.float32)
    out = np.zeros(16, np.uint8)
    soft = np.zeros(64 * 2, np.float32)
    # the decoder produces no information bytes
    assert L.pcg_decode_f32(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None) == U
    assert L.pcg_decode_f32_host(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None) == U
    assert L.pcg_decode_f32_soft(p._h, zf.ctypes.data, 2, out.ctypes.data, None, soft.ctypes.data, None) == U
    assert L.pcg_decode_f32_soft_host(p._h, zf.ctypes.data, 2, out.ctypes.data, None, soft.ctypes.data) == U
    assert L.pcg_decode_i8(p._h, z8.ctypes.data, 2, out.ctypes.data, None, None, None) == U
    assert L.pcg_decode_i8_host(p._h, z8.ctypes.data, 2, out.ctypes.data, None, None) == U
    punc = nat.Puncturer(60, fr, device=-1)
    assert L.pcg_decode_punctured_f32(p._h, punc._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None) == U
    # the SCAN, Fast-SSCAN and SC-Flip entry points refuse an error-locator plan
    assert L.pcg_decode_scan_f32_host(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None) == A
    assert L.pcg_decode_scan_f32(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None, None) == A
    assert L.pcg_plan_set_scan_iterations(p._h, 2) == A
    assert L.pcg_decode_fsscan_f32_host(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None) == A
    assert L.pcg_decode_fsscan_f32(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None, None) == A
    assert L.pcg_plan_set_fsscan_trials(p._h, 2, 0) == A
    assert L.pcg_decode_depthfirst_f32_host(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None) == A
    assert L.pcg_decode_depthfirst_f32(p._h, zf.ctypes.data, 2, out.ctypes.data, None, None, None, None) == A
    assert L.pcg_plan_set_depthfirst_trials(p._h, 2) == A


def test_locating_on_another_plan_is_an_argument_error():
    nat = _nat()
    L = nat.lib()
    fr = frozen_bits(64, 32, 0.0)
    z = np.zeros((2, 64), np.float32)
    first = np.zeros(2, np.int32)
    for p in (nat.Plan(64, 1, fr, device=-1), nat.ScanPlan(64, 1, fr, device=-1),
              nat.FastSscanPlan(64, 1, fr, device=-1), nat.DepthFirstPlan(64, 1, fr, device=-1)):
        assert L.pcg_errorlocator_f32_host(p._h, 1, z.ctypes.data, None, 2, None, None, first.ctypes.data,
                                           None) == nat.PCG_E_ARG
        assert L.pcg_errorlocator_f32(p._h, 1, z.ctypes.data, None, 2, None, None, first.ctypes.data, None,
                                      None) == nat.PCG_E_ARG


def test_host_only_plan_fails_loudly():
    nat = _nat()
    p = nat.ErrorLocatorPlan(64, frozen_bits(64, 32, 0.0), device=-1)
    for mode in ("reference", "correct", "first"):
        with pytest.raises(nat.PcgError) as e:
            p.locate_host(np.zeros((2, 64), np.float32), mode=mode)
        assert e.value.code == nat.PCG_E_NODEVICE
    with pytest.raises(nat.PcgError) as e:  # no information bytes on this plan
        nat.Plan.decode_host(p, np.zeros((2, 64), np.float32))
    assert e.value.code == nat.PCG_E_UNSUPPORTED


def test_pypolar_error_locator_without_gpu():
    from antpolarcodes_amd import pypolar
    assert "ErrorLocator" in pypolar.__all__
    fr = frozen_bits(256, 128, 0.0)
    el = pypolar.ErrorLocator(256, fr)
    assert el.blockLength() == 256 and el.infoLength() == 128 and list(el.frozenBits()) == list(fr)
    assert el.firstError() == -1 and el.correctionCount() == 0 and el.getOutput().shape == (256,)
    el.setAsReferenceDecoder()
    el.setDesiredOutput(np.zeros(256, np.float32))
    assert not hasattr(el, "pushBit")
    with pytest.raises(RuntimeError, match="blockLength float32 values"):
        el.setDesiredOutput(np.zeros(255, np.float32))
    with pytest.raises(RuntimeError, match="Only ONE-dimensional vectors allowed!"):
        el.decode_vector(np.zeros((2, 256), np.float32))
    with pytest.raises(RuntimeError, match="Input vector size"):
        el.decodeFindFirstError(np.zeros(255, np.float32))
    with pytest.raises(RuntimeError, match="locate_batch expects"):
        el.locate_batch(np.zeros((2, 255), np.float32))
    with pytest.raises(RuntimeError, match="mode is"):
        el.locate_batch(np.zeros((2, 256), np.float32), mode="genie")
    with pytest.raises(RuntimeError, match="shape of the frames"):
        el.locate_batch(np.zeros((2, 256), np.float32), np.zeros((3, 256), np.float32))
    for bad in ((100, [0, 1]), (64, list(range(64))), (64, [3, 2]), (8192, [0])):
        with pytest.raises(Exception):
            pypolar.ErrorLocator(*bad)
    if _nat().device_count() <= 0:  # decoding without a GPU fails loudly
        with pytest.raises(RuntimeError, match="no HIP device"):
            el.decode_vector(np.zeros(256, np.float32))
        with pytest.raises(RuntimeError, match="no HIP device"):
            el.locate_batch(np.zeros((2, 256), np.float32))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_error_locator_class_through_the_reference_header(tmp_path):
    """tests/cpp/errorlocator_caller.cpp builds ErrorLocator(1024, frozen) through
    <polarcode/decoding/errorlocator.h>."""
    exe = str(tmp_path / "errorlocator_caller")
    src = os.path.join(ROOT, "tests", "cpp", "errorlocator_caller.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", LIB, "-lpolarcode_amd", "-lpcg", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "api"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert "errorlocator api ok" in r.stdout


# ---- the errorlocator tool with a mocked backend ------------------------------------------------

def test_tool_options_and_job():
    from antpolarcodes_amd import errorlocator as tool
    a = tool.parser().parse_args([])
    assert (a.workload, a.snr, a.design_snr, a.blocklength, a.rate, a.output, a.threads) == \
        (10000, 2.0, 0.0, 1024, 0.5, "badbits", 1)
    a = tool.parser().parse_args(["--workload", "7", "--snr", "1.5", "--design-snr", "1", "--blocklength", "64",
                                  "--rate", "0.25", "--output", "x", "--threads", "2"])
    assert (a.workload, a.snr, a.design_snr, a.blocklength, a.rate, a.output, a.threads) == (7, 1.5, 1.0, 64, 0.25,
                                                                                              "x", 2)
    job = tool.Job(tool.parser().parse_args(["-n", "1024", "-w", "100000"]))
    assert (job.N, job.K, job.BlocksToSimulate) == (1024, 512, 100000)
    assert job.frozen == frozen_bits(1024, 512, 0.0, "BB") and job.frozenSet.sum() == 512
    assert tool.file_name("badbits", job) == "badbits_1024_512_2.000000.csv"
    job = tool.Job(tool.parser().parse_args(["-n", "256", "-r", "0.3", "-s", "2.5", "-d", "1.0", "-w", "1001", "-t",
                                             "4"]))
    assert job.K == int(np.float32(256) * np.float32(0.3)) == 76 and job.BlocksToSimulate == 250
    assert job.frozen == frozen_bits(256, 76, 1.0, "BB")
    assert tool.file_name("out", job) == "out_256_76_2.500000.csv"
    # K = int(N * rate) in float32: 0.7f is just below 0.7, 10 * 0.7f rounds to 7.0f in float32
    assert tool.Job(tool.parser().parse_args(["-n", "128", "-r", "0.7"])).K == int(np.float32(128) * np.float32(0.7))


class Mock:
    """A backend that replays recorded (first, count) blocks."""

    def __init__(self, blocks):
        self.blocks, self.calls, self.closed = list(blocks), [], False

    def setup(self, job):
        self.N = job.N

    def block(self, job, F, seed):
        self.calls.append((F, seed))
        first, count = self.blocks.pop(0)
        assert len(first) == F
        return np.array(first, np.int32), np.array(count, np.uint32)

    def close(self):
        self.closed = True


def test_tool_counts_and_writes_the_reference_csv(tmp_path):
    """Counting as countErrors, and a CSV whose statistics columns are the reference's recorded
    strings: position p receives the recorded sequence k as its correction counts, in order."""
    from antpolarcodes_amd import errorlocator as tool
    z = gold()
    nseq = int(z["stat_count"][0])
    seqs = [z[f"stat{k}_values"].astype(int).tolist() for k in range(nseq)]
    job = tool.Job(tool.parser().parse_args(["-n", "64", "-r", "0.5", "-w", "200", "-s", "1.0"]))
    info = np.flatnonzero(~job.frozenSet)
    pos = [int(info[3 * k]) for k in range(nseq)]
    first, count = [], []
    for j in range(max(len(s) for s in seqs)):  # interleaved, so that order within a position matters
        for k, s in enumerate(seqs):
            if j < len(s):
                first.append(pos[k])
                count.append(s[j])
    first += [-1] * (200 - len(first))  # frames without a correction
    count += [0] * (200 - len(count))
    mock = Mock([(first[:128], count[:128]), (first[128:], count[128:])])
    lines = []
    tool.run(job, batch=128, make_backend=lambda w: mock, log=lines.append)
    assert [c[0] for c in mock.calls] == [128, 72] and mock.closed and job.runs == 200
    assert lines == ["[1] N=64, K=32, dSNR=0.000000, SNR=1.000000", "[1] Finished"]
    for k, s in enumerate(seqs):
        assert job.firstErrorPosition[pos[k]] == len(s) and job.additionalErrors[pos[k]] == [float(v) for v in s]
    assert job.firstErrorPosition.sum() == sum(len(s) for s in seqs)
    path = tmp_path / tool.file_name("badbits", job)
    assert path.name == "badbits_64_32_1.000000.csv"
    tool.save_results(job, str(path))
    rows = path.read_text().splitlines()
    assert rows[0] == '"Index","Frozen","First error histogram","Mean additional","Dev add","Min add","Max add"'
    assert len(rows) == 65
    for bit in range(64):
        cols = rows[1 + bit].split(",")
        assert cols[0] == str(bit) and cols[1] == ('"F"' if job.frozenSet[bit] else '"I"')
        if bit in pos:
            k = pos.index(bit)
            assert cols[2] == str(len(seqs[k])) and cols[3:] == z[f"stat{k}_str"].tolist(), (bit, cols)
        else:
            assert cols[2:] == ["0", "0", "0", "0", "0"]


def test_tool_workers_share_the_job():
    from antpolarcodes_amd import errorlocator as tool
    job = tool.Job(tool.parser().parse_args(["-n", "64", "-w", "21", "-t", "2"]))
    assert job.BlocksToSimulate == 10
    i = int(np.flatnonzero(~job.frozenSet)[0])
    mocks = [Mock([([i] * 10, [2] * 10)]), Mock([([i] * 10, [3] * 10)])]
    tool.run(job, batch=64, make_backend=lambda w: mocks[w])
    assert job.runs == 20 and job.firstErrorPosition[i] == 20
    assert sorted(job.additionalErrors[i]) == [2.0] * 10 + [3.0] * 10
    assert {c[1] for m in mocks for c in m.calls} == {1000003, 2000006}  # each worker its own seed
