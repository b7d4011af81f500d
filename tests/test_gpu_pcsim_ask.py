"""pcsim's `ask` simulation type on the GPU: jobs whose frames go through the ASK channel kernel
(modulate, AWGN, demodulate, Scale(amplification) in one launch) and the GPU decoders; their block /
bit / reported error counts must equal the oracle's decisions on the very same LLRs.

Both jobs: -n 256 -r 0.5 -e crc8, 3000 frames.  Eb/N0 was chosen on the CPU beforehand (the numpy
model of tests/ask_numpy.py with numpy's normal noise, 3000 frames, decoded by the oracle) so that
the block error rate lies between 0.02 and 0.5:

  bitsPerSymbol 3 (256 is not divisible by 3), -l 1 -p 32:  Eb/N0 = 7 dB, CPU-side BLER 0.190
                                                            (6 dB: 0.478, 8 dB: 0.039)
  bitsPerSymbol 2, -l 4 -p 832:                             Eb/N0 = 4 dB, CPU-side BLER 0.248
                                                            (3 dB: 0.643, 5 dB: 0.046)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class Recording:
    """GpuBackend that keeps every batch's LLRs and sent info bytes (as in test_gpu_pcsim.py)."""

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
        self.be.close()


@pytest.mark.parametrize("bps,L,precision,ebn0", [(3, 1, 32, 7.0), (2, 4, 832, 4.0)])
def test_pcsim_ask_job_matches_oracle(oracle, bps, L, precision, ebn0):
    from antpolarcodes_amd import pcsim
    N = 256
    a = pcsim.parser().parse_args(["ask", "-n", str(N), "-r", "0.5", "-l", str(L), "-p", str(precision), "-e", "crc8",
                                   "-w", str(N * 3000), "--snr-max", str(ebn0), "--snr-count", "8"])
    # snr-count 8: the last point of each modulation order is --snr-max itself
    job = [j for j in pcsim.build_jobs(a) if j.bitsPerSymbol == bps][-1]
    assert (job.EbN0, job.bitsPerSymbol, job.N, job.K, job.L, job.channel) == (ebn0, bps, N, 128, L, "awgn")
    rec = Recording()
    pcsim.run_job(job, rec, batch=1024, seed=5)
    llr = np.concatenate(rec.llr[1:])  # the first call is the warm-up batch
    sent = np.concatenate(rec.sent[1:])
    assert llr.shape == (3000, N) and job.runs == 3000
    fr = rec.frozen
    if precision == 832:  # AdaptiveMixed: FastSscFipChar on the quantised floats, then SclAvxFloat
        info, ok = oracle.scc_decode(N, fr, llr, crc=8)
        bad = np.nonzero(ok == 0)[0]
        if bad.size:
            info[bad], ok[bad] = oracle.scl_decode(N, L, fr, llr[bad], crc=8)
    else:
        info, ok = oracle.sc_decode(N, fr, llr, crc=8)
    be = np.unpackbits(np.bitwise_xor(sent, info), axis=1).sum(axis=1)
    print(f"ask job b={bps} L={L} p={precision}: BLER {job.BLER:.4f} at {ebn0} dB")
    assert job.errors == int((be > 0).sum())
    assert job.biterrors == int(be.sum())
    assert job.reportedErrors == int((ok == 0).sum())
    assert 0 < job.BLER < 1
