"""Times the streaming receive loop (gmr1_hip_rx_stream_*) against one gmr1_hip_rx_run_dev call: 64 BCCH carriers of
--seconds at sps 4 (8 synthetic carriers, each used for 8 ARFCNs), device-resident, pushed through one handle in 10 ms,
100 ms and 1 s pushes (push_dev, one stream).  Reports per push the host wall time around the call (a push is
synchronous: that includes its host work and its copies back) and the device time on its stream (events recorded before and
after the call: from its first device operation to its last, gaps where the stream waits for the push's host part
included); median and p99 over the last three quarters of the pushes, the maximum over all; then the total of a pass against the one-shot call, and the
real-time factor (capture seconds per second of the pass).  Then the chained pipeline: a wideband capture through
ChanStream.push_dev -> RxStream.push_dev on one stream, against channelize + rx_run.  Checks the records are identical.
--tch: every carrier has a traffic carrier with one call on it (an IMMEDIATE ASSIGNMENT around frame 40, some ciphered),
the handle follows TCH3 calls (push_tch_dev) and the one-shot call is gmr1_hip_rx_run_tch_dev; the chained pipeline is
left out.
--full: every carrier also has a CSD carrier with one data call on it (an ASSIGNMENT COMMAND 1 on the call's FACCH3 from
call frame 25 on), the handle follows TCH3 and TCH9 calls (push_full_dev) and the one-shot call is
gmr1_hip_rx_run_full_dev; records and big records are compared, the chained pipeline is left out.
--voice: --tch's capture through a handle that also decodes the calls (push_voice_dev) against gmr1_hip_rx_run_voice_dev,
records and audio blocks compared; every push size is also run through a tch handle in the same process, the passes
alternating, and "voice_extra_ms" is the voice push's median time over the tch push's (wall and device).

    python tools/time_rx_stream.py [--seconds 60] [--pushes 0.01,0.1,1] [--tch | --voice | --full] [--wide-seconds 0] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _sorted(rec, arfcn):
    pos = {int(a): i for i, a in enumerate(arfcn)}
    key = np.array([pos[int(a)] * 256 + int(c) for a, c in zip(rec["arfcn"], rec["chain"])], np.int64)
    return rec[np.argsort(key, kind="stable")] if len(rec) else rec


def finish(res, out):
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--pushes", default="0.01,0.1,1", help="push lengths in seconds")
    ap.add_argument("--wide-seconds", type=float, default=10.0,
                    help="length of the chained pipeline's wideband capture (0: leave the pipeline out)")
    ap.add_argument("--tch", action="store_true", help="follow TCH3 calls: one call per carrier")
    ap.add_argument("--full", action="store_true", help="follow TCH3 and TCH9 calls: one voice and one data call per carrier")
    ap.add_argument("--voice", action="store_true", help="follow TCH3 calls and decode them: --tch's capture, audio blocks out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.tch + args.full + args.voice > 1:
        ap.error("--tch, --voice and --full are three kinds of handle: give one")
    voice = args.voice
    args.tch = args.tch or voice           # a voice handle takes what a tch handle takes
    import torch
    import workloads
    from __graft_entry__ import load_package
    pkg = load_package()
    api = pkg.api
    torch.cuda.init()
    api.load()
    api.init(0)
    sps, A, rate = 4, 64, 23400 * 4
    kc = dt = dc = None
    if args.full:
        import oracle_lib as orc
        orc.build()
        orc.lib()
        keys = [np.arange(8, dtype=np.uint8) + k if k % 2 else None for k in range(8)]
        pairs = [workloads.bcch_tch_csd_triple(pkg, orc, 900 + k, seconds=args.seconds, sps=sps, stn=(7 * k) % 32, delay=k % 8,
                                               tn=(5 * k + 3) % 32, p=(7 * k) % 40, tn9=(3 * k + 2) % 24, k_ass=40, k_cmd=25, kc=keys[k],
                                               cfo_hz=40.0 * k - 150.0)[:3] for k in range(8)]
        base = [b for b, _, _ in pairs]
        kc = np.stack([keys[i % 8] if keys[i % 8] is not None else np.zeros(8, np.uint8) for i in range(A)])
    elif args.tch:
        keys = [np.arange(8, dtype=np.uint8) + k if k % 2 else None for k in range(8)]
        pairs = [workloads.bcch_tch_pair(pkg, 900 + k, seconds=args.seconds, sps=sps, stn=(7 * k) % 32, delay=k % 8, tn=(5 * k + 3) % 32,
                                         p=(7 * k) % 40, k_ass=40, kc=keys[k], cipher_after=None if keys[k] is None else 25,
                                         cfo_hz=40.0 * k - 150.0)[:2] for k in range(8)]
        base = [b for b, _ in pairs]
        kc = np.stack([keys[i % 8] if keys[i % 8] is not None else np.zeros(8, np.uint8) for i in range(A)])
    else:
        base = [workloads.bcch_carrier(pkg, 900 + k, seconds=args.seconds, sps=sps, stn=(7 * k) % 32, delay=k % 8,
                                       cfo_hz=40.0 * k - 150.0, esn0_db=10.0 + k)[0] for k in range(8)]
    n = min(x.size for x in base)
    x = np.stack([base[i % 8][:n] for i in range(A)]).astype(np.complex64)
    arfcn = np.arange(A, dtype=np.uint16) + 100
    d = torch.from_numpy(x.view(np.float32).reshape(A, -1)).cuda()
    if args.tch or args.full:
        dt = torch.from_numpy(np.stack([pairs[i % 8][1][:n] for i in range(A)]).astype(np.complex64).view(np.float32).reshape(A, -1)).cuda()
    if args.full:
        dc = torch.from_numpy(np.stack([pairs[i % 8][2][:n] for i in range(A)]).astype(np.complex64).view(np.float32).reshape(A, -1)).cuda()
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    offset = np.arange(A, dtype=np.uint64) * np.uint64(n)
    length = np.full(A, n, np.uint64)
    res = {"carriers": A, "capture_s": n / rate, "sps": sps, "tch": bool(args.tch), "full": bool(args.full), "voice": bool(voice)}
    out = np.empty(1 << 21, api.RX_RECORD)
    ref_big = ref_audio = None
    if voice:
        def one_shot():
            rec, audio, status, chains, _, n_audio = api.rx_run_voice_dev(st, d.data_ptr(), dt.data_ptr(), offset, length, sps=sps,
                                                                          arfcn=arfcn, kc=kc, max_records=1 << 21, max_audio=1 << 18)
            assert n_audio == len(audio)
            return (rec, audio), status, chains, None
    elif args.full:
        def one_shot():
            rec, big, status, chains = api.rx_run_full_dev(st, d.data_ptr(), dt.data_ptr(), dc.data_ptr(), offset, length, sps=sps,
                                                           arfcn=arfcn, kc=kc, max_records=1 << 21, max_big=1 << 20)
            return (rec, big), status, chains, None
    elif args.tch:
        one_shot = lambda: api.rx_run_tch_dev(st, d.data_ptr(), dt.data_ptr(), offset, length, sps=sps, arfcn=arfcn, kc=kc,
                                              max_records=1 << 21)
    else:
        one_shot = lambda: api.rx_run_dev(st, d.data_ptr(), offset, length, sps=sps, arfcn=arfcn, out=out)
    one_shot()      # warm-up
    t = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref, rst, rch, _ = one_shot()
        t.append(time.perf_counter() - t0)
    if args.full:
        ref, ref_big = ref
        res["big_records"] = int(len(ref_big))
    if voice:
        ref, ref_audio = ref
        res["audio_blocks"] = int(len(ref_audio))
        res["audio_speech_blocks"] = int(np.sum(ref_audio["cls"] == 4))
    ref = ref.copy()
    res["one_shot_ms"] = 1e3 * min(t)
    res["records"] = int(len(ref))
    res["tch_records"] = int(np.sum(ref["type"] >= 0x10))
    for p_s in [float(v) for v in args.pushes.split(",")]:
        p = int(round(p_s * rate))
        best = best_tch = None
        # (with --voice the passes alternate: tch handle, voice handle, tch handle, voice handle)
        for rep_i in range(4 if voice else 2):
            as_voice = voice and rep_i % 2 == 1
            per, got, got_big, evs = [], [], [], []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with api.RxStream(A, sps=sps, arfcn=arfcn, tch=args.tch and not as_voice, full=args.full, voice=as_voice, kc=kc) as s:
                at = 0
                buf = np.empty(max(s.max_records(p), 1), api.RX_RECORD)
                bbuf = np.empty(max(s.max_big(p), 1), api.RX_BIG_RECORD)
                abuf = np.empty(max(s.max_audio(p), 1), api.RX_AUDIO) if as_voice else None
                while at < n:
                    k = min(p, n - at)
                    if s.max_records(k) > buf.size:
                        buf = np.empty(s.max_records(k), api.RX_RECORD)
                    if s.max_big(k) > bbuf.size:
                        bbuf = np.empty(s.max_big(k), api.RX_BIG_RECORD)
                    if as_voice and s.max_audio(k) > abuf.size:
                        abuf = np.empty(s.max_audio(k), api.RX_AUDIO)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    q0 = time.perf_counter()
                    if as_voice:
                        r, rb = s.push_dev(st, d.data_ptr() + 8 * at, n, k, last=at + k >= n, out=buf, tch_ptr=dt.data_ptr() + 8 * at,
                                           audio=abuf)
                    elif args.full:
                        r, rb = s.push_dev(st, d.data_ptr() + 8 * at, n, k, last=at + k >= n, out=buf, tch_ptr=dt.data_ptr() + 8 * at,
                                           csd_ptr=dc.data_ptr() + 8 * at, big=bbuf)
                    else:
                        r = s.push_dev(st, d.data_ptr() + 8 * at, n, k, last=at + k >= n, out=buf,
                                       tch_ptr=dt.data_ptr() + 8 * at if args.tch else None)
                    per.append(time.perf_counter() - q0)
                    e1.record(stream)
                    evs.append((e0, e1))
                    got.append(r.copy())
                    if args.full or as_voice:
                        got_big.append(rb.copy())
                    at += k
            total = time.perf_counter() - t0
            torch.cuda.synchronize()
            dev = [a.elapsed_time(b) for a, b in evs]
            if voice and not as_voice:
                if best_tch is None or total < best_tch[0]:
                    best_tch = (total, per, got, dev, got_big)
            elif best is None or total < best[0]:
                best = (total, per, got, dev, got_big)
        total, per, got, dev, got_big = best
        same = _sorted(np.concatenate(got), arfcn).tobytes() == ref.tobytes()
        if args.full:
            same = same and _sorted(np.concatenate(got_big), arfcn).tobytes() == ref_big.tobytes()
        if voice:
            same = same and _sorted(np.concatenate(got_big), arfcn).tobytes() == ref_audio.tobytes()
            same = same and _sorted(np.concatenate(best_tch[2]), arfcn).tobytes() == ref.tobytes()
        per_ms = np.array(per) * 1e3
        dev_ms = np.array(dev)
        steady = per_ms[len(per_ms) // 4:] if len(per_ms) > 8 else per_ms
        steady_dev = dev_ms[len(dev_ms) // 4:] if len(dev_ms) > 8 else dev_ms
        res["push_%gs" % p_s] = {"pushes": len(per), "total_ms": 1e3 * total, "vs_one_shot": total * 1e3 / res["one_shot_ms"],
                                 "rtf": (n / rate) / total, "push_wall_ms_median": float(np.median(steady)),
                                 "push_wall_ms_p99": float(np.percentile(steady, 99)), "push_wall_ms_max": float(per_ms.max()),
                                 "push_dev_ms_median": float(np.median(steady_dev)),
                                 "push_dev_ms_p99": float(np.percentile(steady_dev, 99)),
                                 "push_dev_ms_max": float(dev_ms.max()), "identical": bool(same)}
        if voice:
            t_per, t_dev = np.array(best_tch[1]) * 1e3, np.array(best_tch[3])
            t_steady = t_per[len(t_per) // 4:] if len(t_per) > 8 else t_per
            t_steady_dev = t_dev[len(t_dev) // 4:] if len(t_dev) > 8 else t_dev
            res["push_%gs" % p_s].update({
                "tch_total_ms": 1e3 * best_tch[0], "tch_push_wall_ms_median": float(np.median(t_steady)),
                "tch_push_dev_ms_median": float(np.median(t_steady_dev)),
                "voice_extra_ms": {"wall_median": float(np.median(steady) - np.median(t_steady)),
                                   "dev_median": float(np.median(steady_dev) - np.median(t_steady_dev)),
                                   "total": 1e3 * (total - best_tch[0])}})
        print(json.dumps({("push_%gs" % p_s): res["push_%gs" % p_s]}), flush=True)
    # the chained pipeline
    if args.tch or args.full or args.wide_seconds <= 0:
        return finish(res, args.out)
    fs = 2.0e6
    carriers = tuple((c, dict(stn=(3 * c) % 32, delay=c % 8, cfo_hz=float(c))) for c in (3, 17, 33, 60))
    wide, _ = workloads.wideband_capture(pkg, 5, seconds=args.wide_seconds, carriers=carriers)
    chans = [c for c, _ in carriers]
    nb = api.channelize(wide, fs, chans)
    wa = np.asarray(chans, np.uint16)
    nn = nb.shape[1]
    ref2, _, _, _ = api.rx_run(np.ascontiguousarray(nb).reshape(-1), np.arange(len(chans), dtype=np.uint64) * np.uint64(nn),
                               np.full(len(chans), nn, np.uint64), sps=4, arfcn=wa, max_records=1 << 20)
    w = torch.from_numpy(wide.view(np.float32)).cuda()
    for p_s in (0.01, 0.1):
        p = int(round(p_s * fs))
        got = []
        cs = api.ChanStream(fs, chans)
        rs = api.RxStream(len(chans), sps=4, arfcn=wa)
        o = torch.empty((len(chans), 2 * (cs.out_len(p) + 64)), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        at = 0
        while at < wide.size:
            k = min(p, wide.size - at)
            m = cs.out_len(k)
            cs.push_dev(st, w.data_ptr() + 8 * at, k, o.data_ptr(), o.shape[1] // 2)
            got.append(rs.push_dev(st, o.data_ptr(), o.shape[1] // 2, m, last=at + k >= wide.size).copy())
            at += k
        total = time.perf_counter() - t0
        cs.close()
        rs.close()
        same = _sorted(np.concatenate(got), wa).tobytes() == ref2.tobytes()
        res["pipeline_%gs" % p_s] = {"carriers": len(chans), "capture_s": wide.size / fs, "total_ms": 1e3 * total,
                                     "rtf": (wide.size / fs) / total, "identical": bool(same)}
        print(json.dumps({("pipeline_%gs" % p_s): res["pipeline_%gs" % p_s]}), flush=True)
    try:
        core, _ = api.clock_probe_dev(st, 2000)
        res["core_mhz"] = core
    except Exception:       # noqa: BLE001
        pass
    finish(res, args.out)


if __name__ == "__main__":
    main()
