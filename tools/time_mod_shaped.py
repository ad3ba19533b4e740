"""Times the shaped modulator (gmr1_hip_mod_shaped_batch_dev: burst bits -> demodulator-ready windows, k_shape) into a
device-resident buffer, next to a plain fill of the same output bytes in the same process -- the kernel has no parent to be
compared with, so the fill (torch's, one store per element and nothing else) is its yardstick.

Two shapes: 1 M nt3_speech bursts at sps 4 in 474-sample windows (BASELINE.md configs[4]'s), and 100 k bcch bursts in
1016-sample windows (the headline's).  Per burst: a few samples of jitter, a fraction of a sample, 150 Hz rms carrier
offset, a phase and a level, raised cosine cut at +-5 symbols.  Kernel and fill alternate, events around each, after a
preroll; every round is reported, not only the median.  Reported per shape: milliseconds, output bytes per second, and
the kernel's time over the fill's.

    python tools/time_mod_shaped.py [--rounds 9] [--scale 1.0] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("nt3_speech", 1_000_000, 4, 474), ("bcch", 100_000, 4, 1016))
SYM_RATE = 23400


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9, help="timed rounds (each: the kernel, then the fill)")
    ap.add_argument("--preroll-s", type=float, default=0.5)
    ap.add_argument("--scale", type=float, default=1.0, help="bursts per shape x this (a rehearsal at a small size)")
    ap.add_argument("--span", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    api = load_package().api
    api.load()
    api.init(0)
    stream = torch.cuda.current_stream(dev)
    res = {"span": args.span, "pulse": "rc", "shapes": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for name, n, sps, in_len in SHAPES:
        n = max(int(n * args.scale), 1)
        info = api.burst_info(name)
        rng = np.random.default_rng(3)
        win = in_len - info.len * sps
        to = lambda a: torch.from_numpy(a).to(dev)
        bits = to(rng.integers(0, 2, (n, info.ebits), dtype=np.uint8))
        off = to((np.arange(n, dtype=np.int64) * in_len))
        start = to((win // 2 + rng.integers(-2, 3, n)).astype(np.int32))
        frac = to(rng.uniform(-0.5, 0.5, n).astype(np.float32))
        cfo = to((rng.normal(0.0, 150.0, n) * (2 * np.pi / (SYM_RATE * sps))).astype(np.float32))
        ph = to(rng.uniform(0, 2 * np.pi, n).astype(np.float32))
        gain = to((10.0 ** (rng.normal(0.0, 3.0, n) / 20.0)).astype(np.float32))
        out = torch.empty((n, in_len, 2), device=dev, dtype=torch.float32)
        out_bytes = out.numel() * 4

        def kernel():
            api.mod_shaped_batch_dev(stream.cuda_stream, name, n, sps, api.PULSE_RC, args.span, in_len, bits.data_ptr(), None,
                                     off.data_ptr(), start.data_ptr(), frac.data_ptr(), cfo.data_ptr(), ph.data_ptr(),
                                     gain.data_ptr(), out.data_ptr(), n * in_len)

        def fill():
            out.fill_(1.0)

        t_end = time.perf_counter() + args.preroll_s
        while time.perf_counter() < t_end:
            fill()
            kernel()
            torch.cuda.synchronize()
        nonzero = bool(out.abs().amax().item() > 0)
        rounds = {"kernel": [], "fill": []}
        for _ in range(args.rounds):
            rounds["kernel"].append(timed(kernel))
            rounds["fill"].append(timed(fill))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        r = {"bursts": n, "sps": sps, "in_len": in_len, "output_bytes": out_bytes, "output_nonzero": nonzero,
             "ms_rounds": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
             "ms_median": {k: round(v, 4) for k, v in med.items()},
             "ms_spread": {k: round(float(max(v) - min(v)), 4) for k, v in rounds.items()},
             "output_GB_per_s": {k: round(out_bytes / (v * 1e-3) / 1e9, 1) for k, v in med.items()},
             "kernel_over_fill": round(med["kernel"] / med["fill"], 3)}
        res["shapes"]["%s_%d_sps%d_win%d" % (name, n, sps, in_len)] = r
        print(json.dumps({name: {k: r[k] for k in ("ms_median", "ms_spread", "output_GB_per_s", "kernel_over_fill")}}), flush=True)
        del out, bits
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
