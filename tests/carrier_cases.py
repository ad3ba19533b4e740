"""Closed-loop inputs of the carrier mixer (gmr1_hip_carrier_mix*), shared by tests/test_carrier_host.py (the oracle's
verdict on them, no GPU) and tests/test_gpu_carrier.py (the same schedules made on the device).

A case is one carrier: one or two transmitters, each with the frame rule of synth.synth_bcch_carrier (frame k starts at
t0 + k 24 39 sps and has frame number fn0 + k; sirfn = (fn - delay) & 63: sirfn % 8 == 0 FCCH, == 2 BCCH, else CCCH unless
idle; all on timeslot stn) and payloads from synth.si1_payload / imm_ass_payload's neighbours.  `build` turns it into what
the mixer is fed: per-format payload arrays, one window per burst in a flat window buffer, and the carrier's segment list
sorted by position (the transmitters' segments interleaved), plus the `sent` list per transmitter.  `restate` is the float64
statement of the mixed carrier from synth.shape_bursts / fcch_dual_chirp windows and tests/carrier_ref.py."""
import numpy as np

import carrier_ref

SYM_RATE = 23400
SPAN = 5
BURST_SYMS = 234          # BCCH and DC6
FCCH_SYMS = 117
SEED = 0x5EEDC0DE12345678

# seconds, Es/N0 and carrier offset of the first two are the issue's; the rest (timing, seeds) is chosen so that the
# oracle's receive loop, run on the restatement alone, finds what test_carrier_host.py asks for
CASES = {
    "15dB": dict(sps=4, seconds=2.5, esn0_db=15.0, cfo_hz=120.0, noise_id=3,
                 tx=[dict(seed=1101, stn=3, delay=2, gain=1.0)]),
    "9dB": dict(sps=4, seconds=2.5, esn0_db=9.0, cfo_hz=-300.0, noise_id=4,
                tx=[dict(seed=1102, stn=0, delay=0, gain=1.0)]),
    "two_tx": dict(sps=4, seconds=3.2, esn0_db=18.0, cfo_hz=60.0, noise_id=5,
                   tx=[dict(seed=1103, stn=2, delay=3, gain=1.0, t0=1000),
                       dict(seed=1104, stn=2, delay=3, gain=0.8, t0=1000 + 11 * 39 * 4)]),
    "sps8": dict(sps=8, seconds=2.5, esn0_db=15.0, cfo_hz=100.0, noise_id=6,
                 tx=[dict(seed=1105, stn=6, delay=3, gain=1.0)]),
}


def n_samples(case):
    return int(case["seconds"] * SYM_RATE * case["sps"])


def sigma(case):
    """deviation per component at unit symbol energy: synth_bcch_carrier's convention"""
    return float(np.sqrt(10.0 ** (-case["esn0_db"] / 10.0) / 2.0))


def cfo(case):
    """radians per sample"""
    return 2.0 * np.pi * case["cfo_hz"] / (SYM_RATE * case["sps"])


def _schedule(synth, tx, n, sps, p_idle=0.15):
    """One transmitter's bursts: (bcch l2, positions), (ccch l2, positions), fcch positions, sent.  A burst is sent if its
    whole body lies within the carrier (synth_bcch_carrier's rule); positions are those of the first sample of its window
    (the body: span symbols ahead of symbol 0; the chirp: its sample 0)."""
    rng = np.random.default_rng(tx["seed"])
    frame_len = 24 * 39 * sps
    t0 = tx.get("t0", int(rng.integers(0, frame_len)))
    fn0 = int(rng.integers(0, 1 << 18))
    stn, delay = tx["stn"], tx["delay"]
    n_frames = (n - t0) // frame_len + 1
    fns = fn0 + np.arange(n_frames)
    sirfn = (fns - delay) & 63
    body = (BURST_SYMS + 2 * SPAN) * sps
    at = lambda k: t0 + int(k) * frame_len + stn * 39 * sps
    sent = []
    kf = [k for k in np.nonzero(sirfn % 8 == 0)[0] if at(k) >= 0 and at(k) + FCCH_SYMS * sps <= n]
    for k in kf:
        sent.append(dict(type="fcch", fn=int(fns[k]), pos=at(k)))
    inside = lambda k: at(k) - SPAN * sps >= 0 and at(k) - SPAN * sps + body <= n
    kb = np.array([k for k in np.nonzero(sirfn % 8 == 2)[0] if inside(k)], np.int64)
    l2b = synth.si1_payload(rng, fns[kb], delay, stn)
    other = rng.random(kb.size) < 0.25                     # some BCCH bursts carry another SI: no TDMA position
    l2b[other, 0] = 0x10 | (l2b[other, 0] & 0x07)
    for i, k in enumerate(kb):
        sent.append(dict(type="bcch", fn=int(fns[k]), pos=at(k), l2=l2b[i].copy()))
    kc = np.nonzero((sirfn % 8 != 0) & (sirfn % 8 != 2))[0]
    kc = np.array([k for k in kc[rng.random(kc.size) >= p_idle] if inside(k)], np.int64)
    l2c = rng.integers(0, 256, size=(kc.size, 24), dtype=np.uint8)
    l2c[:, 1] &= 0xF7                                      # never an IMMEDIATE ASSIGNMENT by accident
    for i, k in enumerate(kc):
        sent.append(dict(type="ccch", fn=int(fns[k]), pos=at(k), l2=l2c[i].copy(), k=int(k), imm_ass=None))
    win = lambda ks: np.array([at(k) - SPAN * sps for k in ks], np.int64)
    return (l2b, win(kb)), (l2c, win(kc)), np.array([at(k) for k in kf], np.int64), sent


def build(pkg, name):
    """-> dict: sps, n, sigma, cfo, noise_id, seed; per window kind ("bcch", "ccch", "fcch") the payloads (None for fcch), the
    per-window gain, in_len and where its windows start in the window buffer; seg_src / seg_pos / seg_len sorted by position
    (stable: ties keep transmitter order); seg_iq_len; sent (all transmitters) and sent_by_tx."""
    case = CASES[name]
    sps, n = case["sps"], n_samples(case)
    parts = [_schedule(pkg.synth, tx, n, sps) for tx in case["tx"]]
    gains = [tx["gain"] for tx in case["tx"]]
    burst_len, fcch_len = (BURST_SYMS + 2 * SPAN) * sps, FCCH_SYMS * sps
    kinds, segs, base = {}, [], 0
    for kind, idx, in_len in (("bcch", 0, burst_len), ("ccch", 1, burst_len), ("fcch", 2, fcch_len)):
        pos = np.concatenate([p[idx] if kind == "fcch" else p[idx][1] for p in parts])
        l2 = None if kind == "fcch" else np.concatenate([p[idx][0] for p in parts])
        gain = np.concatenate([np.full((p[idx] if kind == "fcch" else p[idx][1]).size, g, np.float32) for p, g in zip(parts, gains)])
        kinds[kind] = dict(l2=l2, gain=gain, in_len=in_len, base=base, n=pos.size)
        segs += [(base + i * in_len, int(q), in_len) for i, q in enumerate(pos)]
        base += pos.size * in_len
    order = np.argsort(np.array([s[1] for s in segs]), kind="stable")
    segs = [segs[i] for i in order]
    return dict(name=name, sps=sps, n=n, sigma=sigma(case), cfo=cfo(case), noise_id=case["noise_id"], seed=SEED, kinds=kinds,
                seg_src=np.array([s[0] for s in segs], np.uint64), seg_pos=np.array([s[1] for s in segs], np.int64),
                seg_len=np.array([s[2] for s in segs], np.uint32), seg_iq_len=base,
                sent=[s for p in parts for s in p[3]], sent_by_tx=[p[3] for p in parts])


def restate(pkg, b):
    """The mixed carrier in float64 from synth's own windows (its encoders, mapper, shaper and chirp) -> complex64"""
    synth, sps = pkg.synth, b["sps"]
    seg_iq = np.zeros(b["seg_iq_len"], np.complex128)
    for kind, enc, fmt in (("bcch", synth.bcch_encode, "bcch"), ("ccch", synth.ccch_encode, "dc6")):
        k = b["kinds"][kind]
        if k["n"]:
            w = synth.shape_bursts(synth.map_symbols(pkg.api.burst_format(fmt), enc(k["l2"])), sps, 0.0, SPAN)
            assert w.shape == (k["n"], k["in_len"])
            seg_iq[k["base"]:k["base"] + w.size] = (w * k["gain"][:, None]).reshape(-1)
    k = b["kinds"]["fcch"]
    chirp = synth.fcch_dual_chirp(0.32, FCCH_SYMS, sps)
    seg_iq[k["base"]:k["base"] + k["n"] * k["in_len"]] = (k["gain"][:, None] * chirp[None, :]).reshape(-1)
    segs = list(zip(b["seg_src"].tolist(), b["seg_pos"].tolist(), b["seg_len"].tolist()))
    x, _, _, _ = carrier_ref.mix(seg_iq, segs, 0, b["n"], b["sigma"], b["cfo"], b["noise_id"], b["seed"])
    return x.astype(np.complex64)


def verdict(records, sent_by_tx):
    """Per transmitter and burst kind: (kind, bursts found by payload, bursts sent from the first found one on, of those not
    found).  What a receiver has to deliver once it follows a transmitter: every BCCH burst, every CCCH burst but at most one."""
    out = []
    for sent in sent_by_tx:
        for kind, code in (("bcch", 1), ("ccch", 2)):
            got = {bytes(r["l2"]) for r in records if r["type"] == code}
            s = [(x["pos"], bytes(x["l2"])) for x in sent if x["type"] == kind]
            hit = [p for p, l in s if l in got]
            after = [l for p, l in s if hit and p >= min(hit)]
            out.append((kind, len(hit), len(after), sum(l not in got for l in after)))
    return out


def check_records(records, chains, b):
    """What both the oracle on the restatement and the device chain have to give on a case -> the verdict, for printing"""
    import workloads
    assert chains >= 1
    v = verdict(records, b["sent_by_tx"])
    followed = [v[i:i + 2] for i in range(0, len(v), 2) if v[i][1]]
    assert followed, v
    for (_, nb_hit, nb_after, nb_missed), (_, nc_hit, nc_after, nc_missed) in followed:
        assert nb_hit >= 3 and nb_missed == 0, v
        assert nc_hit >= 10 and nc_missed <= 1, v
    mb, nb, mc, nc, mp = workloads.match_records(records, b["sent"])
    assert nb >= 3 and mp == nb and mc >= nc - 1, (mb, nb, mc, nc, mp)
    return v
