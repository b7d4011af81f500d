"""ASK modulation and the --channel option on the CPU: the constants of Ask::setBitsPerSymbol
(pcg_ask_constants), argument checking of pcg_ask_channel_f32, and pcsim's `ask` simulation type
(configureAskSim, simulator.cpp:342-357) with a mocked backend."""
import ctypes as C

import numpy as np
import pytest

import ask_numpy
from antpolarcodes_amd import _native, pcsim


def _args(*argv):
    return pcsim.parser().parse_args(list(argv))


class MockBackend:
    """Random info bytes as frames; the 'decoder' returns them with every 7th frame corrupted."""

    def setup(self, job):
        self.bps = job.bitsPerSymbol

    def frames(self, job, F, seed):
        info = np.random.default_rng(seed).integers(0, 256, (F, job.K // 8), dtype=np.uint8)
        return info.copy(), info, 1e-3

    def decode(self, job, llr):
        got = llr.copy()
        got[::7, 0] ^= 0x11
        return got, np.ones(llr.shape[0], np.uint8), 2e-3

    def close(self):
        pass


@pytest.mark.parametrize("b", range(1, 17))
def test_ask_constants_equal_the_numpy_model(b):
    nm, pn = _native.ask_constants(b)
    enm, epn = ask_numpy.constants(b)
    assert nm.dtype == np.float32 and pn.dtype == np.float32
    assert (nm.view(np.uint32), pn.view(np.uint32)) == (enm.view(np.uint32), epn.view(np.uint32))


def test_ask_constants_known_values():
    assert _native.ask_constants(1) == (1.0, 1.0)
    # b = 2: levels 1, 3 -> power 10, nm = sqrt(2 * 10 / 4)
    nm, pn = _native.ask_constants(2)
    assert nm == np.float32(np.sqrt(5.0)) and pn == np.float32(1.0 / float(np.float32(np.sqrt(5.0))))
    # b = 10: the float32 running sum of 1 + 9 + ... + 1023^2 passes 2^24 and rounds; the exact
    # sum 178956800 gives another normal magnitude than the float one
    power = np.float32(0.0)
    for s in range(1, 1024, 2):
        power = np.float32(power + np.float32(s * s))
    assert float(power) != 178956800.0
    assert _native.ask_constants(10)[0] == np.float32(np.sqrt(2.0 * float(power) / 1024.0))


def test_argument_errors():
    L = _native.lib()
    nm, pn = C.c_float(), C.c_float()
    for b in (0, 17, 1 << 20):
        assert L.pcg_ask_constants(b, C.byref(nm), C.byref(pn)) == _native.PCG_E_ARG
        with pytest.raises(_native.PcgError):
            _native.ask_constants(b)
    assert L.pcg_ask_constants(4, None, C.byref(pn)) == _native.PCG_E_ARG
    assert L.pcg_ask_constants(4, C.byref(nm), None) == _native.PCG_E_ARG
    # the channel call checks before it touches a device: (code, F, n, bps, fading, sigma, gain,
    # seed, out, symbols, stream)
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert L.pcg_ask_channel_f32(p, 1, 8, 0, 0, 0.5, 1.0, 1, p, None, None) == _native.PCG_E_ARG
    assert L.pcg_ask_channel_f32(p, 1, 8, 17, 0, 0.5, 1.0, 1, p, None, None) == _native.PCG_E_ARG
    assert L.pcg_ask_channel_f32(p, 0, 8, 17, 0, 0.5, 1.0, 1, p, None, None) == _native.PCG_E_ARG
    assert L.pcg_ask_channel_f32(p, 1, 8, 2, 2, 0.5, 1.0, 1, p, None, None) == _native.PCG_E_ARG
    assert L.pcg_ask_channel_f32(p, 1, 8, 2, -1, 0.5, 1.0, 1, p, None, None) == _native.PCG_E_ARG
    assert L.pcg_ask_channel_f32(None, 1, 8, 2, 0, 0.5, 1.0, 1, p, None, None) == _native.PCG_E_ARG
    assert L.pcg_ask_channel_f32(p, 1, 8, 2, 1, 0.5, 1.0, 1, None, None, None) == _native.PCG_E_ARG
    assert L.pcg_ask_channel_f32(p, 1, 12, 2, 0, 0.5, 1.0, 1, p, None, None) == _native.PCG_E_ARG
    assert L.pcg_ask_channel_f32(p, 1, 0, 2, 0, 0.5, 1.0, 1, p, None, None) == _native.PCG_E_ARG
    # no frames: nothing to do, also with null buffers
    assert L.pcg_ask_channel_f32(None, 0, 8, 2, 1, 0.5, 1.0, 1, None, None, None) == _native.PCG_OK


def test_configure_ask_gives_nine_modulation_orders():
    jobs = pcsim.configure(_args("ask"))
    assert [j.bitsPerSymbol for j in jobs] == list(range(2, 11))
    t = pcsim.default_job(_args("ask"))
    for j in jobs:  # everything else is the default job
        assert (j.N, j.K, j.L, j.precision, j.errorDetection, j.channel) == (t.N, t.K, t.L, t.precision,
                                                                             t.errorDetection, "awgn")
    assert "ask" in pcsim.SUPPORTED


def test_build_jobs_inflates_ask_over_snr():
    jobs = pcsim.build_jobs(_args("ask", "--snr-count", "8", "-p", "32"))
    # snr-count 8: 1 + 3 + 1 points per template, templates in order
    assert len(jobs) == 9 * 5
    assert [j.bitsPerSymbol for j in jobs] == [b for b in range(2, 11) for _ in range(5)]
    ref = pcsim.build_jobs(_args("single", "--snr-count", "8", "-p", "32"))
    assert [j.EbN0 for j in jobs[:5]] == [j.EbN0 for j in ref]
    assert [j.amplification for j in jobs[5:10]] == [j.amplification for j in ref]


def test_mock_backend_runs_an_ask_job_and_bps_reaches_the_csv(tmp_path):
    jobs = pcsim.build_jobs(_args("ask", "-n", "256", "-w", str(256 * 1000), "--snr-count", "8", "-e", "crc8"))
    job = next(j for j in jobs if j.bitsPerSymbol == 3)
    pcsim.run_job(job, MockBackend(), batch=300, seed=3)
    assert job.runs == 1000 and job.errors == sum(len(range(0, F, 7)) for F in (300, 300, 300, 100))
    out = tmp_path / "r.csv"
    pcsim.save_results([job], str(out))
    lines = out.read_text().splitlines()
    cols = lines[1].split(",")
    assert lines[0].split(",")[6] == '"BPS"' and cols[6] == "3"
    assert cols[:5] == ["256", "128", "0", "8", "8"]


def test_channel_option():
    assert _args().channel == "awgn"
    assert pcsim.default_job(_args()).channel == "awgn"
    a = _args("ask", "--channel", "rayleigh")
    assert a.channel == "rayleigh"
    assert all(j.channel == "rayleigh" for j in pcsim.build_jobs(a))
    with pytest.raises(SystemExit):
        _args("--channel", "rician")


@pytest.mark.parametrize("simtype", ["fixed", "compareall"])
def test_types_needing_the_compiled_in_code_still_exit(simtype):
    with pytest.raises(SystemExit):
        pcsim.configure(_args(simtype))
