"""Captures and helpers of tests/test_gpu_rx_stream_full.py: BCCH carriers with the TCH3 carrier their IMMEDIATE ASSIGNMENTs
point to and the CSD carrier the ASSIGNMENT COMMANDs on its FACCH3 point to, the push loop of a handle that follows both,
and the one-shot reference (gmr1_hip_rx_run_full), computed once per capture and Viterbi decoder mode and shared by the
tests."""
import functools
from importlib import import_module

import numpy as np

import workloads

SPS = 4
FRAME = 24 * 39 * SPS
KC1 = np.arange(8, dtype=np.uint8)
# the three carriers of test_rx_loop_tch9_follow_up_matches_oracle (test_gpu_rxloop.py)
TRIPLES = [dict(seed=2, kc=KC1, mix9=(0.0, 1.0)), dict(seed=3, kc=None, mix9=(0.3, 0.6)), dict(seed=4, kc=KC1, mix9=(0.2, 0.5), tn9=17)]
TWO_SLOTS = [(25, 5), (45, 14)]      # (call frame, timeslot) of the commands of two_slots()


def _stack(parts):
    assert len({v.size for p in parts for v in p[:3]}) == 1
    return dict(x=np.stack([p[0] for p in parts]).astype(np.complex64), t=np.stack([p[1] for p in parts]).astype(np.complex64),
                c=np.stack([p[2] for p in parts]).astype(np.complex64), kc=np.stack([p[3] for p in parts]))


@functools.lru_cache(maxsize=1)
def triples(pkg, orc):
    """-> dict(x, t, c (3, n) complex64, kc (3, 8))"""
    parts = []
    for cs in TRIPLES:
        cs = dict(cs)
        parts.append(workloads.bcch_tch_csd_triple(pkg, orc, cs.pop("seed"), seconds=5.5, sps=SPS, **cs)[:4])
    return _stack(parts)


@functools.lru_cache(maxsize=2)
def at_sps(pkg, orc, sps):
    """one carrier at another sps; the command comes early so that a short capture holds a few dozen NT9 frames"""
    return _stack([workloads.bcch_tch_csd_triple(pkg, orc, 30 + sps, seconds=4.5, sps=sps, k_cmd=8, kc=KC1, mix9=(0.2, 0.7), tn9=9)[:4]])


@functools.lru_cache(maxsize=1)
def two_slots(pkg, orc, seed=7, seconds=5.5, sps=SPS, tn=11, p=20, k_ass=15, esn0_db=25.0, cfo_hz=40.0, mix9=(0.2, 0.8)):
    """One chain whose FACCH3 messages name timeslot 5 from call frame 25 and timeslot 14 from call frame 45 (the list form
    of synth_tch3_carrier's ass_cmd), and a CSD carrier whose NT9 bursts sit on the timeslot the receiver is on: the one
    named by the last command whose message ended (its fourth burst) at or before the frame.  Built as
    workloads.bcch_tch_csd_triple builds its CSD side, with the oracle's encoders (test data only)."""
    synth = import_module(pkg.__name__ + ".synth")
    rng = np.random.default_rng(seed)
    n = int(seconds * 23400 * sps)
    frame_len = 24 * 39 * sps
    t0 = int(rng.integers(0, frame_len))
    fn0 = int(rng.integers(0, 1 << 18))
    fb, fd = pkg.api.burst_format("bcch"), pkg.api.burst_format("dc6")
    fs, ff = pkg.api.burst_format("nt3_speech"), pkg.api.burst_format("nt3_facch")
    f9 = pkg.api.burst_format("nt9")
    bcch, sent = synth.synth_bcch_carrier(fb, fd, n, sps, rng, stn=3, delay=2, fn0=fn0, t0=t0, esn0_db=esn0_db, cfo_hz=cfo_hz,
                                          imm_ass=[(k_ass, tn, p)])
    k_start = [s for s in sent if s["type"] == "ccch" and s.get("imm_ass")][0]["k"]
    tch, sent_t = synth.synth_tch3_carrier(fs, ff, n, sps, rng, t0=t0, fn0=fn0, k_start=k_start, tn=tn, p=p, kc=None, esn0_db=esn0_db,
                                           cfo_hz=cfo_hz, mix=(0.2, 0.2, 0.6), ass_cmd=[(k_start + k, tn9) for k, tn9 in TWO_SLOTS])
    # the timeslot in force per frame: a command takes effect in the frame of its message's fourth burst
    cmds = []
    for s in sent_t:
        l2 = s.get("l2")
        if s["type"] == "facch3" and l2[3] == 0x06 and l2[4] == 0x2E:
            cmds.append((s["k"] + 3, ((int(l2[5]) & 3) << 3) | (int(l2[6]) >> 5)))
    assert {tn9 for _, tn9 in cmds} == {tn9 for _, tn9 in TWO_SLOTS}
    sigma = np.sqrt(10.0 ** (-esn0_db / 10.0) / 2.0)
    csd = (rng.standard_normal((n, 2)) * sigma).astype(np.float32).view(np.complex64).reshape(-1)
    n_frames = (n - t0) // frame_len - 1
    il = orc.Interleaver()
    orc.lib().orc_interleaver_init(orc.C.byref(il), orc.C.c_int(3), orc.C.c_int(648))
    kc = KC1
    span = 5
    for k in range(k_start, n_frames):
        fn = fn0 + k
        on = [tn9 for k_eff, tn9 in cmds if k_eff <= k]
        u = rng.random()
        if not on or u >= mix9[0] + mix9[1]:
            continue
        ciph = synth.a5_1(kc, [fn], 658)[0]
        sacch = rng.integers(0, 2, 10, dtype=np.uint8)
        status = rng.integers(0, 2, 4, dtype=np.uint8)
        if u < mix9[0]:
            l2 = rng.integers(0, 256, 38, dtype=np.uint8)
            l2[37] &= 0x0F
            e = orc.facch9_encode(l2, sacch, status, ciph)
            sid = 0
        else:
            l2 = rng.integers(0, 256, 60, dtype=np.uint8)
            e = np.zeros(662, np.uint8)
            orc.lib().orc_tch9_encode(e.ctypes.data_as(orc.C.c_void_p), l2.ctypes.data_as(orc.C.c_void_p), orc.C.c_int(2),
                                      sacch.ctypes.data_as(orc.C.c_void_p), status.ctypes.data_as(orc.C.c_void_p),
                                      ciph.ctypes.data_as(orc.C.c_void_p), orc.C.byref(il))
            sid = 1
        body = synth.shape_bursts(synth.map_symbols(f9, e[None, :], sync_id=sid), sps, 0.0, span)[0]
        pos = t0 + k * frame_len + on[-1] * 39 * sps - span * sps
        if pos >= 0 and pos + body.size <= n:
            csd[pos:pos + body.size] += body
    if cfo_hz:
        ph = (2 * np.pi * cfo_hz / (23400 * sps)) * np.arange(n, dtype=np.float64)
        csd *= np.exp(1j * ph).astype(np.complex64)
    return _stack([(bcch, tch, csd, kc)])


_ONE_SHOT = {}


def one_shot(api, name, cap, arfcn, sps=SPS):
    """gmr1_hip_rx_run_full on the whole capture, once per (capture, decoder mode) -> (records, big records, status, chains)"""
    key = (name, api.get_conv_decoder(), bytes(np.asarray(arfcn, np.uint16)))
    if key not in _ONE_SHOT:
        A, n = cap["x"].shape
        offset = np.arange(A, dtype=np.uint64) * np.uint64(n)
        length = np.full(A, n, np.uint64)
        rec, big, status, chains = api.rx_run_full(cap["x"].reshape(-1), cap["t"].reshape(-1), cap["c"].reshape(-1), offset, length,
                                                   sps=sps, arfcn=arfcn, kc=cap["kc"], max_records=1 << 20, max_big=1 << 16)
        rec.setflags(write=False)
        big.setflags(write=False)
        _ONE_SHOT[key] = (rec, big, status, chains)
    return _ONE_SHOT[key]


def stream(api, cap, sizes, arfcn, sps=SPS, after_push=None, push=None):
    """push the capture in pieces of the given sizes (the rest in the last one) through a handle that follows TCH3 and TCH9
    calls -> (records, big records, status, n_chains, [(records, big records) of each push]).  push(s, x, t, c, last):
    another way to make the push than RxStream.push."""
    x, t, c = cap["x"], cap["t"], cap["c"]
    A, n = x.shape
    if push is None:
        push = lambda s, xa, ta, ca, last: s.push(xa, tch=ta, csd=ca, last=last)
    got, at = [], 0
    with api.RxStream(A, sps=sps, arfcn=arfcn, full=True, kc=cap["kc"]) as s:
        for k in sizes:
            k = min(int(k), n - at)
            if at + k >= n:
                break
            r, b = push(s, x[:, at:at + k], t[:, at:at + k], c[:, at:at + k], False)
            got.append((r.copy(), b.copy()))
            at += k
            if after_push:
                after_push(s, at)
        r, b = push(s, x[:, at:], t[:, at:], c[:, at:], True)
        got.append((r.copy(), b.copy()))
        status, chains, _ = s.status()
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]), status, chains, got
