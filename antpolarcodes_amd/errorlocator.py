"""The `errorlocator` tool ("bad bit finder") on the GPU:  python -m antpolarcodes_amd.errorlocator

Restates the reference's src/errorlocator (setup.cpp, simulator.cpp, statistics.cpp) around the
batched error-locator kernel.  For every bit index of one code at one SNR it measures how often
plain SC makes its FIRST wrong decision there, and how many further wrong decisions follow once
the earlier ones are corrected by a genie -- what one looks at to design a flip decoder.

  * options and defaults: setup.cpp:24-34 (-w workload 10000, -s snr 2.0, -d design-snr 0.0,
    -n blocklength 1024, -r rate 0.5, -o output "badbits", -t threads 1);
  * the job (Simulator::configure, simulator.cpp:58-99): K = int(N * rate) in float32,
    Bhattacharyya frozen set at the design SNR, blocks = workload / threads per worker;
  * per block (SimulationWorker::run, :153-284): random information, non-systematic encoding,
    BPSK, AWGN at Es/N0 = Eb/N0 * K / N (float32, :195-203), Scale(4 Es/N0); the reference decoder
    (setAsReferenceDecoder) runs on the noiseless +-1 signal and its getOutput() is the desired
    vector of the locating decoder on the noisy signal;
  * countErrors (:272-284): a frame with corrections adds one to firstErrorPosition[first] and
    its correction count to additionalErrors[first];
  * saveResults (:101-125): <output>_<N>_<K>_<std::to_string(float Eb/N0)>.csv with, per bit,
    index, "F" / "I", the first-error histogram and Statistics::evaluate of the counts
    (statistics.cpp:24-61, float32, in frame order) as the stream writes floats.

On the GPU, frames are generated, encoded, transmitted and located in blocks of --batch frames
(pcsim's frame source: pcg_random_info, pcg_encode, pcg_bpsk_awgn_f32 and its scaling); a block
is one reference-mode launch and one correcting launch of errorlocator_kernel, and only `first`
and `count` leave the device.  Worker w runs on GPU w % device_count.
"""
import argparse
import os
import sys
import threading

import numpy as np

from .pcsim import fmt as _fmt

f32 = np.float32
CSV_HEADER = '"Index","Frozen","First error histogram","Mean additional","Dev add","Min add","Max add"'


def parser():
    ap = argparse.ArgumentParser(prog="errorlocator", description="Polar code bad bit finder on MI355X")
    ap.add_argument("-w", "--workload", type=int, default=10000, help="number of blocks to examine")
    ap.add_argument("-s", "--snr", type=float, default=2.0, help="SNR (Eb/N0) in dB")
    ap.add_argument("-d", "--design-snr", type=float, default=0.0)
    ap.add_argument("-n", "--blocklength", type=int, default=1024)
    ap.add_argument("-r", "--rate", type=float, default=0.5)
    ap.add_argument("-o", "--output", default="badbits")
    ap.add_argument("-t", "--threads", type=int, default=1)
    ap.add_argument("--batch", type=int, default=1 << 15, help="frames per GPU launch (this build)")
    return ap


class Job:
    """DataPoint (simulator.h) of the one job the tool runs."""

    def __init__(self, a):
        from .construction import frozen_bits
        self.EbN0 = float(f32(a.snr))
        self.designSNR = float(f32(a.design_snr))
        self.threads = max(1, int(a.threads))
        self.BlocksToSimulate = int(a.workload) // self.threads
        self.N = int(a.blocklength)
        self.K = int(f32(self.N) * f32(a.rate))  # int * float in float32, truncated
        self.frozen = frozen_bits(self.N, self.K, self.designSNR, "BB")
        self.frozenSet = np.zeros(self.N, bool)
        self.frozenSet[list(self.frozen)] = True
        self.firstErrorPosition = np.zeros(self.N, np.int64)
        self.additionalErrors = [[] for _ in range(self.N)]
        self.runs = 0
        self.lock = threading.Lock()


def file_name(output, job):
    """saveResults' file name; std::to_string(float) is "%f"."""
    return f"{output}_{job.N}_{job.K}_{job.EbN0:f}.csv"


def fmt(x):
    """C++ ostream << float with the default precision; NaN as glibc prints it."""
    x = f32(x)
    if np.isnan(x):
        return "-nan" if np.signbit(x) else "nan"
    return _fmt(float(x))


def statistics(values):
    """Statistics::evaluate (statistics.cpp:24-61), float32 in insertion order: (mean, dev, min,
    max).  Nothing inserted: zeros.  The min / max scan is the reference's `if ... else if`; the
    deviation divides by size - 1, so a single value gives sqrt(0 / 0), x86's negative NaN."""
    c = [f32(v) for v in values]
    if not c:
        return f32(0), f32(0), f32(0), f32(0)
    size, mn, mx, s = len(c), 0, 0, f32(0)
    for i in range(size):
        s = f32(s + c[i])
        if c[i] < c[mn]:
            mn = i
        elif c[i] > c[mx]:
            mx = i
    mean = f32(s / f32(size))
    s = f32(0)
    for v in c:
        t = f32(v - mean)
        s = f32(s + f32(t * t))
    if size == 1:
        dev = np.array([0xFFC00000], np.uint32).view(f32)[0]
    else:
        dev = f32(np.sqrt(f32(s / f32(size - 1))))
    return mean, dev, c[mn], c[mx]


def count_errors(job, first, count):
    """countErrors (:272-284) over a block, in frame order."""
    first, count = np.asarray(first), np.asarray(count)
    with job.lock:
        job.runs += int(first.shape[0])
        for f in np.flatnonzero(count > 0):
            job.firstErrorPosition[first[f]] += 1
            job.additionalErrors[first[f]].append(float(count[f]))


def save_results(job, path):
    """saveResults (:101-125)."""
    with open(path, "w") as fh:
        fh.write(CSV_HEADER + "\n")
        for bit in range(job.N):
            mean, dev, mn, mx = statistics(job.additionalErrors[bit])
            fh.write(f"{bit}," + ('"F"' if job.frozenSet[bit] else '"I"') + f",{int(job.firstErrorPosition[bit])},"
                     f"{fmt(mean)},{fmt(dev)},{fmt(mn)},{fmt(mx)}\n")


class GpuBackend:
    """One worker's device: pcsim's frame source and the error-locator plan, on one HIP stream.
    `hook(llr, desired)`, when set, receives every block's device tensors before they are located."""

    def __init__(self, device=0, hook=None):
        import torch
        self.torch = torch
        self.device = device
        self.dev = torch.device(f"cuda:{device}")
        self.hook = hook

    def setup(self, job):
        from ._native import Encoder, ErrorLocatorPlan
        self.enc = Encoder(job.N, job.frozen, systematic=False, crc=0, device=self.device)
        self.plan = ErrorLocatorPlan(job.N, job.frozen, device=self.device)
        # setChannel (:195-203), float32
        esn0 = f32(f32(f32(10.0 ** (job.EbN0 / 10.0)) * f32(job.K)) / f32(job.N))
        self.sigma = float(np.sqrt(1.0 / (2.0 * float(esn0))))
        # the device channel returns 2 y / sigma^2; the reference locates Scale(4 Es/N0) y
        self.scale = float(f32(4.0 * float(esn0))) * self.sigma * self.sigma / 2.0

    def block(self, job, F, seed):
        with self.torch.cuda.device(self.dev):
            return self._block(job, F, seed)

    def _block(self, job, F, seed):
        torch = self.torch
        from ._native import bpsk_awgn_device, random_info_device
        kb = (job.K + 7) // 8
        info = torch.empty((F, kb), dtype=torch.uint8, device=self.dev)
        code = torch.empty((F, job.N // 8), dtype=torch.uint8, device=self.dev)
        clean = torch.empty((F, job.N), dtype=torch.float32, device=self.dev)
        llr = torch.empty((F, job.N), dtype=torch.float32, device=self.dev)
        desired = torch.empty((F, job.N), dtype=torch.float32, device=self.dev)
        first = torch.empty(F, dtype=torch.int32, device=self.dev)
        count = torch.empty(F, dtype=torch.int32, device=self.dev)
        random_info_device(info, job.K, seed)
        self.enc.encode_device(info, code)
        bpsk_awgn_device(code, job.N, 0.0, 0, clean)  # the reference signal: noiseless +-1
        bpsk_awgn_device(code, job.N, self.sigma, seed ^ 0x9E3779B97F4A7C15, llr)
        llr.mul_(self.scale)
        self.plan.locate(clean, None, "reference", u=desired)
        if self.hook is not None:
            self.hook(llr, desired)
        self.plan.locate(llr, desired, "correct", first=first, count=count)
        return first.cpu().numpy(), count.cpu().numpy()

    def close(self):
        for p in (getattr(self, "plan", None), getattr(self, "enc", None)):
            if p is not None:
                p.close()


def run_worker(job, backend, worker_id, batch, log=None):
    """SimulationWorker::run (:153-175) for one worker, in blocks of `batch` frames."""
    if log:  # jobStartingOutput (:286-300)
        log(f"[{worker_id}] N={job.N}, K={job.K}, dSNR={job.designSNR:f}, SNR={job.EbN0:f}")
    backend.setup(job)
    done, k = 0, 0
    while done < job.BlocksToSimulate:
        F = min(batch, job.BlocksToSimulate - done)
        first, count = backend.block(job, F, worker_id * 1000003 + k)
        count_errors(job, first, count)
        done += F
        k += 1
    backend.close()
    if log:  # jobEndingOutput (:302-312)
        log(f"[{worker_id}] Finished")


def run(job, batch=1 << 15, make_backend=None, log=None):
    """Simulator::run (:29-54): `threads` workers, worker w on GPU w % device_count."""
    if make_backend is None:
        from ._native import device_count
        ng = max(1, device_count())

        def make_backend(w):
            return GpuBackend(w % ng)
    errors = []

    def worker(w):
        try:
            run_worker(job, make_backend(w), w + 1, batch, log)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(w,)) for w in range(job.threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errors:
        raise errors[0]
    return job


def main(argv=None):
    a = parser().parse_args(argv)
    job = Job(a)
    run(job, batch=a.batch, log=lambda m: print(m, flush=True))
    path = file_name(a.output, job)
    save_results(job, path)
    print(f"results: {os.path.abspath(path)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
