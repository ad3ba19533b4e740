"""Traffic carriers and expected results of the batched TCH3 call follower (gmr1_hip_tch3_follow_batch*), shared by
tests/test_gpu_tch3_follow.py and tests/test_tch3_follow_host.py.  What a call has to report is put together here from
the CPU oracle's primitives in the order gmr1_rx runs them per frame (rx_tch3, _rx_tch3_dkab, _rx_tch3_facch,
_rx_tch3_facch_flush, _rx_tch3_speech; reference src/gmr1_rx.c:378-600)."""
import ctypes as C
import functools

import numpy as np

SYM_RATE = 23400
MARGIN = 0.05          # how far from its threshold every energy decision of the test carriers has to stay
OFF, DKAB, DKAB_MISSING, FACCH, SPEECH, ERR = range(6)
NEED_NONE, NEED_SPEECH, NEED_FLUSH = range(3)

# the five parameter sets; between them every class occurs, a ciphering switch, and a call that ends (ten DKAB_MISSING, then OFF)
CASES = [
    dict(sps=4, seed=1, seconds=2.0, tn=11, p=20),
    dict(sps=4, seed=2, seconds=2.0, tn=4, p=7, mix=(0.2, 0.3, 0.5), cipher_from=10),
    dict(sps=4, seed=3, seconds=2.0, tn=9, p=12, k_stop=20),
    dict(sps=2, seed=4, seconds=1.5, tn=20, p=33),
    dict(sps=10, seed=5, seconds=1.5, tn=0, p=0),
]
CIPHERED = 1           # index of the case whose carrier is ciphered from frame 10 on
ENDING = 2             # index of the case whose carrier stops at frame 20
f32 = np.float32


def in_len(sps):
    return 117 * sps + sps + sps // 2


def burst_energy(win):
    """gmr1_rx.c:172-182 in single precision: the samples len>>5 .. len-(len>>5), summed in order, over len"""
    n = win.size
    b = n >> 5
    v = win[b:n - b]
    n2 = (v.real.astype(f32) * v.real.astype(f32) + v.imag.astype(f32) * v.imag.astype(f32)).astype(f32)
    return f32(np.cumsum(n2, dtype=f32)[-1] / f32(n))


@functools.lru_cache(maxsize=None)
def carrier(pkg, idx):
    """-> dict: the carrier of CASES[idx] alone (samples x), what it carries (sent), its key, and the per-frame inputs of the
    follower: offset (into x), freq_shift, fn"""
    c = CASES[idx]
    sps = c["sps"]
    rng = np.random.default_rng(7000 + c["seed"])
    n = int(c["seconds"] * SYM_RATE * sps)
    frame_len = 24 * 39 * sps
    t0 = int(rng.integers(0, frame_len))
    fn0 = int(rng.integers(0, 1 << 18))
    kc = rng.integers(0, 256, 8, dtype=np.uint8)
    cfo_hz = 60.0
    fs, ff = pkg.api.burst_format("nt3_speech"), pkg.api.burst_format("nt3_facch")
    x, sent = pkg.synth.synth_tch3_carrier(fs, ff, n, sps, rng, t0=t0, fn0=fn0, k_start=0, tn=c["tn"], p=c["p"], kc=kc,
                                           cipher_from=c.get("cipher_from"), cfo_hz=cfo_hz,
                                           mix=c.get("mix", (0.35, 0.35, 0.3)), k_stop=c.get("k_stop"))
    il = in_len(sps)
    e_toa = (il - 117 * sps) >> 1
    offset, fn = [], []
    k = 0
    while t0 + k * frame_len + 2 * frame_len <= n:
        begin = t0 + k * frame_len + sps * c["tn"] * 39 - e_toa
        if begin >= 0 and begin + il <= n:               # burst_map: a window that does not fit is not handed in
            offset.append(begin)
            fn.append(fn0 + k)
        k += 1
    nf = len(offset)
    return dict(idx=idx, sps=sps, in_len=il, e_toa=e_toa, p=c["p"], kc=kc, x=x.astype(np.complex64), sent=sent,
                offset=np.array(offset, np.uint64), fn=np.array(fn, np.uint32),
                freq_shift=np.full(nf, -2.0 * np.pi * cfo_hz / SYM_RATE, np.float32), cipher_from_fn=fn0 + c.get("cipher_from", 1 << 30))


def initial_state(pkg, car, kc=None, p=None):
    """tch3_state_assign(p, ref_energy = 1.0) on a zeroed state that holds the key"""
    st = np.zeros(1, pkg.api.TCH3_STATE)
    st["kc"][0] = car["kc"] if kc is None else kc
    return pkg.api.tch3_state_assign(st, car["p"] if p is None else p, 1.0)


@functools.lru_cache(maxsize=None)
def _burst_results(pkg, orc, idx):
    car = carrier(pkg, idx)
    sps, il = car["sps"], car["in_len"]
    out = []
    for off, fs, fn in zip(car["offset"], car["freq_shift"], car["fn"]):
        w = car["x"][int(off):int(off) + il]
        det = orc.detect(["nt3_facch", "nt3_speech"], float(car["e_toa"]), w, sps, float(fs))
        fa = orc.demod("nt3_facch", w, sps, float(fs))
        sp = orc.demod("nt3_speech", w, sps, float(fs))
        out.append(dict(energy=burst_energy(w), det_rv=det["rv"], btid=det["bt_id"], facch_rv=fa["rv"], facch_sid=fa["sync_id"],
                        facch_eb=fa["ebits"], speech_rv=sp["rv"], speech_eb=sp["ebits"], fn=int(fn)))
    return out


@functools.lru_cache(maxsize=None)
def frame_results(pkg, orc, idx, p=None):
    """Everything the follower computes per frame before it decides, from the oracle: list of dicts(energy, dkab_rv, det_rv,
    btid, facch_rv, facch_sid, facch_eb, speech_rv, speech_eb, fn).  p: the DKAB position searched (default: the carrier's)"""
    car = carrier(pkg, idx)
    pp = car["p"] if p is None else p
    return [dict(r, dkab_rv=orc.dkab_demod(car["x"][int(off):int(off) + car["in_len"]], car["sps"], float(fs), pp)[0])
            for r, off, fs in zip(_burst_results(pkg, orc, idx), car["offset"], car["freq_shift"])]


def _facch3_decode(orc, ebits, ciph):
    l2, s = np.zeros(10, np.uint8), np.zeros(32, np.uint8)
    eb = np.ascontiguousarray(ebits, np.int8)
    cv = C.c_int()
    f = orc.lib().orc_facch3_decode
    f.restype = C.c_int
    crc = f(l2.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), eb.ctypes.data_as(C.c_void_p),
            None if ciph is None else np.ascontiguousarray(ciph, np.uint8).ctypes.data_as(C.c_void_p), C.byref(cv))
    return l2, crc, cv.value


def expected(pkg, orc, idx, state=None, kc=None, lo=0, hi=None, p=None):
    """rx_tch3 over frames lo..hi of CASES[idx], starting from `state` (default: initial_state).  In the Viterbi decoder mode
    the oracle is in.  -> (slots: TCH3_FRAME array, margins: relative distance of every energy decision from its threshold,
    steps: (cls, need, flush) per frame, the state afterwards)"""
    car = carrier(pkg, idx)
    res = frame_results(pkg, orc, idx, p)[lo:hi]
    st = (initial_state(pkg, car, kc, p) if state is None else np.array(state, pkg.api.TCH3_STATE, ndmin=1))[0].copy()
    key = np.array(st["kc"], np.uint8)
    slots = np.zeros(len(res), pkg.api.TCH3_FRAME)
    margins, steps = [], []

    def flush(slot, fn):
        ks = [orc.a5(1, key, int(st["bi_fn"][i]), 96)[0] for i in range(4)]
        ciph = np.concatenate(ks) if st["ciph"] else None
        l2, crc, conv = _facch3_decode(orc, st["ebits"], ciph)
        used = int(st["ciph"])
        if not st["ciph"] and crc:                       # retry with ciphering
            l2, crc, conv = _facch3_decode(orc, st["ebits"], np.concatenate(ks))
            used = 1
            if not crc:
                st["ciph"] = 1
        if not crc:
            slot["type"], slot["len"], slot["ciph"], slot["fn"], slot["conv"] = 0x12, 10, used, (fn - 3) & 0xffffffff, conv
            slot["l2"][:10] = l2
        st["sync_id"] ^= 1
        st["burst_cnt"] = 0
        st["bi_fn"][:] = 0xffffffff
        st["ebits"][:] = 0

    for r, slot in zip(res, slots):
        be = f32(r["energy"])
        slot["energy"] = be
        if not st["active"]:
            slot["cls"] = OFF
            steps.append((OFF, NEED_NONE, 0))
            continue
        det = f32((f32(st["energy_dkab"]) + f32(st["energy_burst"])) / f32(4.0))
        margins.append(abs(float(be) - float(det)) / float(det))
        if be < det:
            rv = r["dkab_rv"]
            slot["cls"] = ERR if rv < 0 else DKAB_MISSING if rv == 1 else DKAB
            steps.append((int(slot["cls"]), NEED_NONE, 0))
            if rv < 0:
                continue
            if rv == 1:
                st["weak_cnt"] += 1
                if st["weak_cnt"] - 1 > 8:
                    st["active"] = 0
            else:
                st["energy_dkab"] = f32(f32(0.1) * be) + f32(f32(0.9) * f32(st["energy_dkab"]))
            continue
        st["weak_cnt"] = 0
        st["energy_burst"] = f32(f32(0.1) * be) + f32(f32(0.9) * f32(st["energy_burst"]))
        fn = r["fn"]
        if r["det_rv"] < 0 or (r["btid"] == 0 and r["facch_rv"] < 0) or (r["btid"] != 0 and r["speech_rv"] < 0):
            slot["cls"] = ERR
            steps.append((ERR, NEED_NONE, 0))
            continue
        if r["btid"] == 0:
            slot["cls"] = FACCH
            bi = fn & 3
            flushed = 0
            if r["facch_sid"] != st["sync_id"]:
                flush(slot, fn)
                flushed = 1
            st["ebits"][104 * bi:104 * bi + 104] = r["facch_eb"]
            st["sync_id"] = r["facch_sid"]
            st["bi_fn"][bi] = fn
            st["burst_cnt"] += 1
            if st["burst_cnt"] == 4:
                assert not flushed
                flush(slot, fn)
                flushed = 2
            steps.append((FACCH, NEED_FLUSH if flushed else NEED_NONE, flushed))
        else:
            slot["cls"] = SPEECH
            ciph = orc.a5(1, key, fn, 208)[0] if st["ciph"] else None
            f0, f1, _, c0, c1 = orc.tch3_decode(r["speech_eb"][None, :], 0, None if ciph is None else ciph[None, :])
            slot["type"], slot["len"], slot["ciph"], slot["fn"] = 0x10, 20, int(st["ciph"]), fn
            slot["conv"] = np.array([(int(c0[0]) & 0xffff) | ((int(c1[0]) & 0xffff) << 16)], np.uint32).view(np.int32)[0]
            slot["l2"][:10], slot["l2"][10:] = f0[0], f1[0]
            steps.append((SPEECH, NEED_SPEECH, 0))
    out_state = np.zeros(1, pkg.api.TCH3_STATE)
    out_state[0] = st
    return slots, margins, steps, out_state


def pack(cars):
    """-> (flat complex64 of the carriers back to back, first, offset, freq_shift, fn) of one call per carrier"""
    base, pos = [], 0
    for c in cars:
        base.append(pos)
        pos += (c["x"].size + 15) & ~15
    iq = np.zeros(pos, np.complex64)
    for b, c in zip(base, cars):
        iq[b:b + c["x"].size] = c["x"]
    first = np.concatenate([[0], np.cumsum([c["offset"].size for c in cars])]).astype(np.int32)
    offset = np.concatenate([c["offset"] + np.uint64(b) for b, c in zip(base, cars)]).astype(np.uint64)
    return iq, first, offset, np.concatenate([c["freq_shift"] for c in cars]), np.concatenate([c["fn"] for c in cars])


def energy_tol(n_in_len, frames_walked=0):
    """Relative bound on an energy against the single-precision restatement: a sum of in_len non-negative float32 terms is,
    in any order, within (in_len - 1) 2^-24 of the exact sum -- two such sums differ by at most twice that -- and every
    0.1 be + 0.9 e of a running average adds two roundings on each side."""
    return (2.0 * n_in_len + 4.0 * frames_walked) * 2.0 ** -24


def call_args(api):
    """A well-formed one-call, two-frame invocation over host arrays: dict of numpy arrays (out filled with 0x55)"""
    return dict(iq=np.zeros(4096, np.complex64), first=np.array([0, 2], np.int32), off=np.array([0, 1000], np.uint64),
                fs=np.zeros(2, np.float32), fn=np.arange(2, dtype=np.uint32), state=np.zeros(1, api.TCH3_STATE),
                out=np.full(80, 0x55, np.uint8).view(api.TCH3_FRAME))


def bad_argument_cases(a):
    """-> (good keyword arguments over the arrays of call_args, the changes both entries refuse with -EINVAL)"""
    p = lambda k: a[k].ctypes.data
    good = dict(n_calls=1, sps=4, in_len=474, iq=p("iq"), iq_len=4096, first=p("first"), n_frames=2, off=p("off"), fs=p("fs"),
                fn=p("fn"), state=p("state"), out=p("out"))
    bad = [dict(sps=0), dict(sps=17), dict(in_len=467), dict(in_len=4097), dict(n_calls=-1), dict(n_frames=-1), dict(iq=None),
           dict(first=None), dict(off=None), dict(fs=None), dict(fn=None), dict(state=None), dict(out=None), dict(iq=p("iq") + 4)]
    return good, bad
