"""Times the carrier mixer (gmr1_hip_carrier_mix_dev, k_carrier_mix) at BASELINE.md configs[3]'s shape -- 64 carriers x 60 s
at four samples per symbol, 2.9 GB of complex64 -- with device-resident inputs and outputs, next to torch's fill and torch's
normal_() of the same bytes in the same process (the kernel has no parent to be compared with: the fill is the store floor,
normal_() another generator's price for the same samples), and next to the host path it replaces (synth.synth_bcch_carrier
for one carrier, extrapolated to all of them).

Every carrier has a full schedule on the 24-slot / 40 ms grid: per 8 frames one FCCH chirp, one BCCH burst and six CCCH
slots (15 % idle), windows of 244 sps samples from gmr1_hip_mod_shaped_batch_dev (random burst bits: only the time is
looked at here) and of 117 sps samples from gmr1_hip_fcch_chirp_batch_dev.  Eight distinct window sets serve the 64
carriers (each carrier has its own timing and its own noise stream).  Three variants alternate with the two yardsticks,
events around --reps launches of each (a single launch is a millisecond: too short a window), after a preroll that lets the
clocks settle; every round is reported, per launch:
    full        sigma != 0, cfo != 0
    cfo0        sigma != 0, cfo == 0 (no fp64)
    noise_only  no segments, cfo == 0

    python tools/time_carrier.py [--rounds 9] [--reps 10] [--carriers 64] [--seconds 60] [--out result.json] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYM_RATE, SPS, SPAN = 23400, 4, 5
DISTINCT = 8


def schedule(rng, n, stn):
    """positions of the (bcch, ccch, fcch) windows of one carrier of n samples: synth_bcch_carrier's frame rule"""
    frame = 24 * 39 * SPS
    t0 = int(rng.integers(0, frame))
    k = np.arange((n - t0) // frame + 1)
    sirfn = (int(rng.integers(0, 1 << 18)) + k) & 63
    at = t0 + k * frame + stn * 39 * SPS
    burst = (234 + 2 * SPAN) * SPS
    ok = (at - SPAN * SPS >= 0) & (at - SPAN * SPS + burst <= n)
    bcch = at[(sirfn % 8 == 2) & ok] - SPAN * SPS
    cc = (sirfn % 8 != 0) & (sirfn % 8 != 2) & ok & (rng.random(k.size) >= 0.15)
    fcch = at[(sirfn % 8 == 0) & (at + 117 * SPS <= n)]
    return bcch, at[cc] - SPAN * SPS, fcch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10, help="launches between the two events of a timed round")
    ap.add_argument("--preroll-s", type=float, default=2.0)
    ap.add_argument("--carriers", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy path (one carrier of --seconds)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    pkg = load_package()
    api = pkg.api
    api.load()
    api.init(0)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    A, n = args.carriers, int(args.seconds * SYM_RATE * SPS)
    rng = np.random.default_rng(3)
    burst, chirp = (234 + 2 * SPAN) * SPS, 117 * SPS

    # the window sets: enough windows of each kind for the busiest carrier, made on the device
    sched = [schedule(rng, n, int(rng.integers(0, 24))) for _ in range(A)]
    n_b, n_c, n_f = (max(len(s[i]) for s in sched) for i in range(3))
    per_set = (n_b + n_c) * burst + n_f * chirp
    seg_iq = torch.zeros(2 * DISTINCT * per_set, device=dev, dtype=torch.float32)
    for d in range(DISTINCT):
        base = d * per_set
        for fmt, cnt, lo in (("bcch", n_b, base), ("dc6", n_c, base + n_b * burst)):
            bits = to(rng.integers(0, 2, (cnt, api.burst_info(fmt).ebits), dtype=np.uint8))
            off = to(lo + np.arange(cnt, dtype=np.int64) * burst)
            start = to(np.full(cnt, SPAN * SPS, np.int32))
            api.mod_shaped_batch_dev(st, fmt, cnt, SPS, api.PULSE_RC, SPAN, burst, bits.data_ptr(), None, off.data_ptr(),
                                     start.data_ptr(), None, None, None, None, seg_iq.data_ptr(), DISTINCT * per_set)
            torch.cuda.synchronize()
        off = to(base + (n_b + n_c) * burst + np.arange(n_f, dtype=np.int64) * chirp)
        api.fcch_chirp_batch_dev(st, "fcch", n_f, SPS, chirp, off.data_ptr(), None, None, None, None, None, seg_iq.data_ptr(),
                                 DISTINCT * per_set)
        torch.cuda.synchronize()
    # the segment lists: carrier c draws on set c % DISTINCT
    first, src, pos, ln = [0], [], [], []
    for c, (pb, pc, pf) in enumerate(sched):
        base = (c % DISTINCT) * per_set
        segs = [(base + i * burst, int(q), burst) for i, q in enumerate(pb)]
        segs += [(base + (n_b + i) * burst, int(q), burst) for i, q in enumerate(pc)]
        segs += [(base + (n_b + n_c) * burst + i * chirp, int(q), chirp) for i, q in enumerate(pf)]
        segs.sort(key=lambda s: s[1])
        src += [s[0] for s in segs]; pos += [s[1] for s in segs]; ln += [s[2] for s in segs]
        first.append(len(src))
    d_first, d_src, d_pos, d_len = to(np.array(first, np.int32)), to(np.array(src, np.int64)), to(np.array(pos, np.int64)), to(np.array(ln, np.int32))
    d_off, d_length = to(np.arange(A, dtype=np.int64) * n), to(np.full(A, n, np.int64))
    d_sigma = to(np.full(A, np.sqrt(10.0 ** -1.5 / 2.0), np.float32))
    d_cfo = to(2 * np.pi * rng.normal(0.0, 150.0, A) / (SYM_RATE * SPS))
    out = torch.empty((A, n, 2), device=dev, dtype=torch.float32)
    out_bytes = out.numel() * 4

    def mix(segments, cfo):
        s = (seg_iq.data_ptr(), d_first.data_ptr(), d_src.data_ptr(), d_pos.data_ptr(), d_len.data_ptr(), burst) if segments else (None,) * 5 + (0,)
        return lambda: api.carrier_mix_dev(st, A, *s, d_off.data_ptr(), d_length.data_ptr(), n, None, d_sigma.data_ptr(),
                                           d_cfo.data_ptr() if cfo else None, None, 7, out.data_ptr())

    work = {"full": mix(True, True), "cfo0": mix(True, False), "noise_only": mix(False, False),
            "fill": lambda: out.fill_(1.0), "normal_": lambda: out.normal_()}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    t_end = time.perf_counter() + args.preroll_s
    while time.perf_counter() < t_end:
        for fn in work.values():
            fn()
        torch.cuda.synchronize()
    work["full"]()
    torch.cuda.synchronize()
    power = float((out[0].double() ** 2).sum(-1).mean().item())
    rounds = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, fn in work.items():
            rounds[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    res = {"carriers": A, "seconds": args.seconds, "reps": args.reps, "sps": SPS, "samples_per_carrier": n, "segments": len(src),
           "window_bytes": int(seg_iq.numel() * 4), "output_bytes": out_bytes, "mean_power_carrier0": round(power, 5),
           "ms_rounds": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_spread": {k: round(float(max(v) - min(v)), 4) for k, v in rounds.items()},
           "output_GB_per_s": {k: round(out_bytes / (v * 1e-3) / 1e9, 1) for k, v in med.items()},
           "over_fill": {k: round(med[k] / med["fill"], 3) for k in med}}
    print(json.dumps({k: res[k] for k in ("ms_median", "ms_spread", "output_GB_per_s", "over_fill")}), flush=True)
    if not args.no_host:
        # the path this replaces: numpy on one host core, one carrier, then the upload; extrapolated to all carriers
        t0 = time.perf_counter()
        x, _ = pkg.synth.synth_bcch_carrier(api.burst_format("bcch"), api.burst_format("dc6"), n, SPS, np.random.default_rng(5),
                                            esn0_db=15.0, cfo_hz=120.0)
        t1 = time.perf_counter()
        to(x.view(np.float32))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res["host_path"] = {"synth_one_carrier_s": round(t1 - t0, 3), "upload_one_carrier_s": round(t2 - t1, 4),
                            "extrapolated_all_carriers_s": round((t2 - t0) * A, 1)}
        print(json.dumps(res["host_path"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
