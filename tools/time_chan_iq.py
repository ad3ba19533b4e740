"""Times the channelizer on integer captures (gmr1_hip_channelize_iq*) against the float entry, on bench.py's chan
workload: 20 s of a 2.0 Msps capture -> all 64 ARFCN streams at sps 4, in one process.

The capture is drawn as int8; its int16 twin is the same values x 256 and its float twin the same values x 2^-7, so the
three formats hold the same samples and their outputs must be identical: checked, and reported as "identical".

  device  : gmr1_hip_channelize_iq_dev on device-resident captures, F32, S16 and S8 alternating, events around each call,
            after a preroll; every round is reported, not only the median.
  host    : gmr1_hip_channelize_iq from host arrays (the upload is the format's bytes), a host clock around the
            synchronous call.
  --parent-lib PATH : a library built from the parent commit; its gmr1_hip_channelize_dev is timed alternately with this
            tree's, to show whether the float path moved.
  --only s16 --calls N : nothing timed, N device-resident calls in one format (for a kernel trace of that call).

    python tools/time_chan_iq.py [--seconds 20] [--rounds 7] [--host-rounds 3] [--parent-lib PATH] [--out result.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("f32", "s16", "s8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=7, help="timed device-resident rounds (each: F32, S16, S8)")
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--preroll-s", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, choices=NAMES)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    api = load_package().api
    api.load()
    api.init(0)
    fs, sps = 2.0e6, 4
    n_in = int(args.seconds * fs) // 64 * 64
    n_chans, _, n_out = api.channelize_plan(fs, sps, n_in)
    chans = list(range(n_chans))
    rng = np.random.default_rng(1)
    h8 = np.clip(np.rint(rng.standard_normal((n_in, 2), dtype=np.float32) * 10.0), -128, 127).astype(np.int8)
    host = {"s8": h8, "s16": h8.astype(np.int16) * 256, "f32": h8.astype(np.float32) * np.float32(2.0 ** -7)}
    fmt = {"f32": api.IQ_F32, "s16": api.IQ_S16, "s8": api.IQ_S8}
    wide = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    outs = {k: torch.empty((n_chans, n_out, 2), device=dev, dtype=torch.float32) for k in NAMES}
    stream = torch.cuda.current_stream(dev)
    res = {"capture_s": n_in / fs, "n_in": n_in, "streams": n_chans, "sps": sps,
           "input_bytes": {k: int(v.nbytes) for k, v in host.items()}}

    def call(k):
        api.channelize_iq_dev(stream.cuda_stream, fmt[k], wide[k].data_ptr(), n_in, fs, chans, outs[k].data_ptr(), n_out, sps=sps)

    if args.only:
        for _ in range(args.calls):
            call(args.only)
        torch.cuda.synchronize()
        return

    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        out_p = torch.empty((n_chans, n_out, 2), device=dev, dtype=torch.float32)
        ch = np.array(chans, np.int32)

        def call_parent():
            rc = parent.gmr1_hip_channelize_dev(C.c_void_p(stream.cuda_stream), C.c_double(fs), sps, C.c_void_p(wide["f32"].data_ptr()),
                                                C.c_uint64(n_in), C.c_float(0.0), ch.size, ch.ctypes.data_as(C.c_void_p),
                                                C.c_void_p(out_p.data_ptr()), C.c_uint64(n_out), None)
            assert rc == 0, rc

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # (as bench.py: calls repeated for --preroll-s first, so that the clocks have ramped up before anything is timed)
    t_end = time.perf_counter() + args.preroll_s
    while time.perf_counter() < t_end:
        for k in NAMES:
            call(k)
        if parent:
            call_parent()
        torch.cuda.synchronize()
    res["identical"] = bool(torch.equal(outs["f32"], outs["s16"]) and torch.equal(outs["f32"], outs["s8"]))
    res["output_nonzero"] = bool(outs["f32"].abs().max().item() > 0)
    if parent:
        res["identical_to_parent"] = bool(torch.equal(outs["f32"], out_p))
    rounds = {k: [] for k in NAMES}
    if parent:
        rounds["f32_parent"] = []
    for _ in range(args.rounds):
        for k in NAMES:
            rounds[k].append(timed(lambda: call(k)))
        if parent:
            rounds["f32_parent"].append(timed(call_parent))
    res["device_ms_rounds"] = {k: [round(v, 4) for v in r] for k, r in rounds.items()}
    res["device_ms_median"] = {k: round(float(np.median(r)), 4) for k, r in rounds.items()}
    res["device_ms_spread"] = {k: round(float(max(r) - min(r)), 4) for k, r in rounds.items()}
    print(json.dumps({k: res[k] for k in ("identical", "device_ms_median", "device_ms_spread")}), flush=True)

    hrounds = {k: [] for k in NAMES}
    same = True
    ref = None
    for i in range(args.host_rounds + 1):                  # (the first round untimed: buffers and pages touched once)
        for k in NAMES:
            x = host[k].view(np.complex64).reshape(-1) if k == "f32" else host[k]
            t0 = time.perf_counter()
            o = api.channelize_iq(x, fs, chans, sps=sps)
            dt = (time.perf_counter() - t0) * 1e3
            if i:
                hrounds[k].append(round(dt, 2))
            else:
                ref = o if ref is None else ref
                same = same and np.array_equal(o, ref)
            del o
    res["host_ms_rounds"] = hrounds
    res["host_ms_median"] = {k: round(float(np.median(r)), 2) for k, r in hrounds.items()}
    res["host_identical"] = bool(same)
    print(json.dumps({k: res[k] for k in ("host_identical", "host_ms_median")}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
