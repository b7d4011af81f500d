"""Time the ASK channel kernel on device-resident code bits: python -m antpolarcodes_amd.channel_time

HIP events around pcg_ask_channel_f32 on 2^16 frames of 1024 random code bits already on the GPU,
3 warm-ups, the median of 20 runs, for b = 1, 2, 3, 4, 10 bits per symbol on AWGN and b = 2 on
Rayleigh.  pcg_bpsk_awgn_f32 is timed alongside on the same bits: every run of a configuration is
preceded by one run of that kernel, so each line carries both medians taken under the same
conditions.  One JSON line per configuration and repeat (--repeats, default 1; five repeats give the
run-to-run spread); GB/s is over the algorithmic bytes F (n/8 + 4n).  Needs a GPU: there is no
fallback.
"""
import argparse
import json
import statistics

CONFIGS = [(1, "awgn"), (2, "awgn"), (3, "awgn"), (4, "awgn"), (10, "awgn"), (2, "rayleigh")]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--sigma", type=float, default=0.5)
    a = ap.parse_args()

    import torch

    from ._native import ask_channel_device, bpsk_awgn_device

    if not torch.cuda.is_available():
        raise SystemExit("channel_time: no GPU")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    code = torch.randint(0, 256, (a.frames, a.n // 8), dtype=torch.uint8, device=dev, generator=gen)
    out = torch.empty((a.frames, a.n), dtype=torch.float32, device=dev)
    ref = torch.empty((a.frames, a.n), dtype=torch.float32, device=dev)
    nbytes = a.frames * (a.n // 8 + 4 * a.n)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    for rep in range(a.repeats):
        for b, fading in CONFIGS:
            ms, ms_ref = [], []
            for r in range(a.warmup + a.runs):
                tr = timed(lambda: bpsk_awgn_device(code, a.n, a.sigma, 7, ref))
                tk = timed(lambda: ask_channel_device(code, a.n, b, a.sigma, 1.0, 7, out, fading=fading))
                if r >= a.warmup:
                    ms.append(tk)
                    ms_ref.append(tr)
            med, med_ref = statistics.median(ms), statistics.median(ms_ref)
            print(json.dumps({"kernel": "ask_channel_kernel", "bits_per_symbol": b, "fading": fading, "n": a.n,
                              "frames": a.frames, "repeat": rep, "ms": round(med, 4),
                              "GBps": round(nbytes / (med * 1e-3) / 1e9, 1), "bpsk_awgn_ms": round(med_ref, 4),
                              "bpsk_awgn_GBps": round(nbytes / (med_ref * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
