"""Times the streaming channelizer (gmr1_hip_chan_stream_*) against the one-shot call on bench.py's chan workload:
20 s of a 2.0 Msps capture -> all 64 ARFCN streams, once in one gmr1_hip_channelize_dev call, then pushed through one
handle in 10 ms, 100 ms and 1 s chunks (push_dev, device-resident, one stream).  Reports per-push device time (events
around each push; the first push of a handle, which grows its buffers to the chunk's size, apart), the aggregate against the
one-shot (all pushes of the fastest of --passes passes, and the steady-state pushes scaled to the whole capture), and the
real-time factor (capture seconds per wall second of that pass); checks that the streamed outputs equal the one-shot's.

    python tools/time_chan_stream.py [--seconds 20] [--chunks 0.01,0.1,1] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--chunks", default="0.01,0.1,1", help="chunk lengths in seconds")
    ap.add_argument("--reps", type=int, default=5, help="one-shot repetitions timed")
    ap.add_argument("--passes", type=int, default=3, help="timed streamed passes per chunk size (a fresh handle each)")
    ap.add_argument("--preroll-s", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    api = load_package().api
    api.load()
    api.init(0)
    fs = 2.0e6
    n_in = int(args.seconds * fs) // 64 * 64
    n_chans, _, n_out = api.channelize_plan(fs, 4, n_in)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    wide = torch.randn((n_in, 2), generator=g, device=dev, dtype=torch.float32)
    ref = torch.empty((n_chans, n_out, 2), device=dev, dtype=torch.float32)
    out = torch.empty_like(ref)
    chans = list(range(n_chans))
    stream = torch.cuda.current_stream(dev)
    res = {"capture_s": n_in / fs, "n_in": n_in, "streams": n_chans}

    def oneshot():
        api.channelize_dev(stream.cuda_stream, wide.data_ptr(), n_in, fs, chans, ref.data_ptr(), n_out)
    # (as bench.py: the one-shot call repeated for --preroll-s first, so that the clocks have ramped up before anything is timed)
    t_end = time.perf_counter() + args.preroll_s
    while time.perf_counter() < t_end:
        oneshot()
        torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    for _ in range(args.reps):
        oneshot()
    ev1.record(stream)
    torch.cuda.synchronize()
    one_ms = ev0.elapsed_time(ev1) / args.reps
    res["oneshot_ms"] = one_ms
    print(json.dumps({"oneshot_ms": round(one_ms, 3)}), flush=True)

    for cs_s in (float(c) for c in args.chunks.split(",")):
        k = int(round(cs_s * fs))
        sizes = [k] * (n_in // k) + ([n_in % k] if n_in % k else [])
        # a first pass warms the code objects; then timed passes, each through a fresh handle (its first push grows the
        # handle's buffers to the chunk's size: reported apart from the steady state)
        passes = []
        for timed in [False] + [True] * args.passes:
            h = api.ChanStream(fs, chans)
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in sizes] if timed else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pos = done = 0
            for i, m in enumerate(sizes):
                if timed:
                    evs[i][0].record(stream)
                done += h.push_dev(stream.cuda_stream, wide.data_ptr() + 8 * pos, m, out.data_ptr() + 8 * done, n_out)
                if timed:
                    evs[i][1].record(stream)
                pos += m
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            h.close()
            assert done == n_out
            if timed:
                same = bool(torch.equal(out, ref))
                per = np.array([a.elapsed_time(b) for a, b in evs])
                passes.append((wall, evs[0][0].elapsed_time(evs[-1][1]), per, same))
        best = min(range(len(passes)), key=lambda i: passes[i][0])
        wall, dev_total, per, _ = passes[best]
        steady = per[1:] if per.size > 1 else per
        r = {"chunk_s": cs_s, "pushes": len(sizes), "passes": len(passes),
             "first_push_ms": float(per[0]), "push_ms_median": float(np.median(steady)),
             "push_ms_p99": float(np.percentile(steady, 99)), "push_ms_max": float(steady.max()),
             "device_ms_total": dev_total, "wall_ms_total": wall * 1e3,
             "device_ms_total_each_pass": [p[1] for p in passes],
             "aggregate_vs_oneshot": dev_total / one_ms, "wall_vs_oneshot": wall * 1e3 / one_ms,
             "aggregate_steady_vs_oneshot": float(steady.sum() * len(sizes) / steady.size) / one_ms,
             "realtime_factor": (n_in / fs) / wall, "identical_to_oneshot": all(p[3] for p in passes)}
        res["chunk_%g" % cs_s] = r
        print(json.dumps({k2: (round(v, 4) if isinstance(v, float) else v) for k2, v in r.items()}), flush=True)
        if not r["identical_to_oneshot"]:
            print("MISMATCH against the one-shot call", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
