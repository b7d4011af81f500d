"""Time the SCAN, the Fast-SSCAN, the SC-Flip or the error-locator kernel on device-resident frames:
python -m antpolarcodes_amd.scan_time [--decoder {scan,fastsscan,depthfirst,errorlocator}]

HIP events around ScanPlan.decode_device (or FastSscanPlan.decode_device) on AWGN frames already
on the GPU (N = 1024, K = 512, CRC-8, 2^14 frames by default), 3 warm-ups, the median of 20 runs,
at 1 and 4 iterations (fastsscan: trial limits; depthfirst: trial limits 1 and 8), with info and ok
only and again with the soft codeword (depthfirst: the decoded words).  Prints one JSON line per
configuration; for fastsscan and depthfirst it also carries the mean number of passes (trials) run
per frame.

errorlocator: the correcting mode on the same AWGN frames; the desired values come from a
reference-mode launch on the noiseless +-1 codewords, which is not timed.  Once with `first` and
`count` only and again with the leaf values `u`; the line carries the mean corrections per frame.
"""
import argparse
import json
import statistics

import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--frames", type=int, default=1 << 14)
    ap.add_argument("--iterations", type=int, nargs="+", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--ebn0", type=float, default=2.0)
    ap.add_argument("--decoder", choices=("scan", "fastsscan", "depthfirst", "errorlocator"), default="scan")
    a = ap.parse_args()
    if a.iterations is None:
        a.iterations = [1, 8] if a.decoder == "depthfirst" else [1, 4]

    import torch

    from . import frames
    from ._native import DepthFirstPlan, ErrorLocatorPlan, FastSscanPlan, ScanPlan
    from .construction import frozen_bits

    fr = frozen_bits(a.n, a.k, 0.0)
    base = min(a.frames, 1024)  # host-generated frames, tiled on the device
    llr, _, code = frames.awgn_frames(a.n, fr, base, a.ebn0, seed=1, crc=8)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(llr)).to(dev).repeat((a.frames + base - 1) // base, 1)[:a.frames]
    x = x.contiguous()
    if a.decoder == "errorlocator":
        return time_errorlocator(a, ErrorLocatorPlan(a.n, fr), x, code, torch)
    fast = a.decoder != "scan"  # detector-terminated: a trial limit, and the trials run come back
    plan = {"scan": ScanPlan, "fastsscan": FastSscanPlan, "depthfirst": DepthFirstPlan}[a.decoder](a.n, 1, fr,
                                                                                                   crc=8)
    info = torch.empty((a.frames, plan.kb), dtype=torch.uint8, device=dev)
    ok = torch.empty((a.frames,), dtype=torch.uint8, device=dev)
    # the soft codeword; depthfirst: the decoded words
    soft = torch.empty((a.frames, a.n), dtype=torch.int32 if a.decoder == "depthfirst" else torch.float32,
                       device=dev)
    trials = torch.empty((a.frames,), dtype=torch.uint8, device=dev) if fast else None
    d = plan.describe()
    for it in a.iterations:
        plan.set_trials(it) if fast else plan.set_iterations(it)
        for want_soft in (False, True):
            ms = []
            for r in range(a.warmup + a.runs):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                plan.decode_device(x, info, ok, soft if want_soft else None, trials)
                t1.record()
                t1.synchronize()
                if r >= a.warmup:
                    ms.append(t0.elapsed_time(t1))
            med = statistics.median(ms)
            line = {"kernel": plan.kernel_name(), "N": a.n, "K": a.k, "frames": a.frames, "iterations": it,
                    "soft": want_soft, "ms": round(med, 4), "cw_per_s": round(a.frames / (med * 1e-3), 1),
                    "ok_rate": round(float(ok.float().mean()), 4), "lds_bytes": d["lds_bytes"],
                    "scratch_bytes_per_codeword": d["scratch_bytes"]}
            if fast:
                line["mean_trials"] = round(float(trials.float().mean()), 4)
            print(json.dumps(line))


def time_errorlocator(a, plan, x, code, torch):
    dev = x.device
    clean = torch.from_numpy((1.0 - 2.0 * code.astype(np.float32)).astype(np.float32)).to(dev)
    clean = clean.repeat((a.frames + clean.shape[0] - 1) // clean.shape[0], 1)[:a.frames].contiguous()
    desired = torch.empty((a.frames, a.n), dtype=torch.float32, device=dev)
    plan.locate(clean, None, "reference", u=desired)  # not timed
    u = torch.empty((a.frames, a.n), dtype=torch.float32, device=dev)
    first = torch.empty((a.frames,), dtype=torch.int32, device=dev)
    count = torch.empty((a.frames,), dtype=torch.int32, device=dev)
    d = plan.describe()
    for want_u in (False, True):
        ms = []
        for r in range(a.warmup + a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            plan.locate(x, desired, "correct", u if want_u else None, None, first, count)
            t1.record()
            t1.synchronize()
            if r >= a.warmup:
                ms.append(t0.elapsed_time(t1))
        med = statistics.median(ms)
        print(json.dumps({"kernel": plan.kernel_name(), "N": a.n, "K": a.k, "frames": a.frames, "mode": "correct",
                          "u": want_u, "ms": round(med, 4), "cw_per_s": round(a.frames / (med * 1e-3), 1),
                          "mean_corrections": round(float(count.float().mean()), 4),
                          "frames_with_corrections": round(float((count > 0).float().mean()), 4),
                          "lds_bytes": d["lds_bytes"], "scratch_bytes_per_codeword": d["scratch_bytes"]}))


if __name__ == "__main__":
    main()
