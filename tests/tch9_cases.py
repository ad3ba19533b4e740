"""Inputs and expected results of the batched TCH9 call follower (gmr1_hip_tch9_follow*), shared by
tests/test_gpu_tch9_follow.py and tests/test_tch9_follow_host.py.  What a call has to report is put together here from
the CPU oracle's primitives in the order gmr1_rx runs them per frame (rx_tch9, reference src/gmr1_rx.c:276-353):
orc.a5, orc.facch9_decode, and orc.tch9_decode_seq over the TCH9 bursts of each call's whole run."""
import functools

import numpy as np

SYM_RATE = 23400
OFF, FACCH9, TCH9, ERR = range(4)
NEED_NONE, NEED_FACCH, NEED_TCH = range(3)
SRC_ZEROS, SRC_HELD0, SRC_HELD1 = -1, -2, -3
TCH9_BYTES = (18, 30, 60)

# the bits form's batch: five calls of 9, 0, 5, 1 and 4 frames (T a TCH9 burst, F a FACCH9 burst, E a window the demodulator
# refused); the 4-burst work-groups of the decoder straddle the call boundaries; the last call is not active
BATCH_KINDS = ["TFTETTFTT", "", "ETTFT", "T", "TFTE"]
NINE = 0               # the call that the continuation tests cut into pieces


# ---- the routing, restated frame by frame (what tch9_follow.h computes as a scan) ----
def classes(active, rv, sync_id):
    return [OFF if not active else ERR if r else FACCH9 if s == 0 else TCH9 for r, s in zip(rv, sync_id)]


def route(active, n_held, rv, sync_id, base=0):
    """-> (cls, need, back-1 source, back-2 source per frame; the carry behind the last frame): a source is a frame index
    (from `base`), SRC_HELD0 / SRC_HELD1, or SRC_ZEROS"""
    last = [SRC_HELD0 if n_held >= 1 else SRC_ZEROS, SRC_HELD1 if n_held >= 2 else SRC_ZEROS]
    out = []
    for k, c in enumerate(classes(active, rv, sync_id)):
        out.append((c, {FACCH9: NEED_FACCH, TCH9: NEED_TCH}.get(c, NEED_NONE), last[0], last[1]))
        if c == TCH9:
            last = [base + k, last[0]]
    return out, tuple(last)


# ---- soft bits ----
def soft(rng, hard):
    """+-127 with 0.3 percent flipped, three percent weakened and 1.5 percent erased: what the punctured rate-3/4 code of
    9k6 still decodes, so that the blocks can also be compared with what was sent"""
    sb = (127 * (1 - 2 * hard.astype(np.int16))).astype(np.int16)
    u = rng.random(sb.shape)
    sb = np.where(u < 0.003, -sb, sb)
    sb = np.where((u >= 0.003) & (u < 0.033), np.sign(sb) * rng.integers(1, 60, sb.shape), sb)
    sb = np.where((u >= 0.033) & (u < 0.048), 0, sb)
    return sb.astype(np.int8)


def taken_in(ebits, ks):
    """A burst as the state holds it: the keystream's sign flips applied, bits_e order, status bits as they are
    (tch9.c:152-160)"""
    e = np.array(ebits, np.int8).astype(np.int16)
    flip = np.zeros(662, bool)
    flip[:52] = ks[:52] != 0
    flip[56:] = ks[52:] != 0
    return np.where(flip, -e, e).astype(np.int8)


def make_call(orc, rng, kinds, mode, kc=None, fn0=None):
    """One call's frames as the demodulator would hand them over -> dict(kc, fn, ebits, sync_id, rv, sent): sent[k] is the L2
    block / message frame k carries (None for E)"""
    kc = rng.integers(0, 256, 8, dtype=np.uint8) if kc is None else np.array(kc, np.uint8)
    fn0 = int(rng.integers(0, 1 << 18)) if fn0 is None else fn0
    n = len(kinds)
    fn = np.arange(fn0, fn0 + n, dtype=np.uint32)
    ks = [orc.a5(1, kc, int(f), 658)[0] for f in fn]
    t_idx = [k for k in range(n) if kinds[k] == "T"]
    nb = TCH9_BYTES[mode]
    blocks = rng.integers(0, 256, (len(t_idx), nb), dtype=np.uint8)
    hard = np.zeros((n, 662), np.uint8)
    if t_idx:
        hard[t_idx] = orc.tch9_encode_seq(blocks, mode, sacch=rng.integers(0, 2, (len(t_idx), 10), dtype=np.uint8),
                                          status=rng.integers(0, 2, (len(t_idx), 4), dtype=np.uint8),
                                          ciph=[ks[k] for k in t_idx])
    sent = [None] * n
    for j, k in enumerate(t_idx):
        sent[k] = blocks[j]
    for k in range(n):
        if kinds[k] == "F":
            l2 = rng.integers(0, 256, 38, dtype=np.uint8)
            l2[37] &= 0x0F
            hard[k] = orc.facch9_encode(l2, rng.integers(0, 2, 10, dtype=np.uint8), rng.integers(0, 2, 4, dtype=np.uint8), ks[k])
            sent[k] = l2
        elif kinds[k] == "E":
            hard[k] = rng.integers(0, 2, 662, dtype=np.uint8)
    return dict(kc=kc, fn=fn, ebits=soft(rng, hard), sync_id=np.array([0 if c == "F" else 1 for c in kinds], np.int32),
                rv=np.array([-1 if c == "E" else 0 for c in kinds], np.int32), sent=sent, kinds=kinds)


def fresh_state(pkg, kc):
    st = np.zeros(1, pkg.api.TCH9_STATE)
    st["kc"][0] = kc
    return pkg.api.tch9_state_assign(st)


def expected_run(pkg, orc, mode, keys, ebits, sync_id, rv, fn):
    """rx_tch9 over one call's whole run from a fresh interleaver, frame k deciphered with keys[k], in the Viterbi decoder
    mode the oracle is in -> (TCH9_FRAME per frame, (n_held, held[1324]) behind every frame: [k] is the state a cut in front
    of frame k passes on, [n] the final one)"""
    n = len(fn)
    slots = np.zeros(n, pkg.api.TCH9_FRAME)
    slots["fn"] = fn
    cls = classes(1, rv, sync_id)
    ks = [orc.a5(1, keys[k], int(fn[k]), 658)[0] if cls[k] in (FACCH9, TCH9) else None for k in range(n)]
    t_idx = [k for k in range(n) if cls[k] == TCH9]
    if t_idx:
        l2, _, _, conv = orc.tch9_decode_seq(np.array([ebits[k] for k in t_idx], np.int8), mode, ciph=[ks[k] for k in t_idx])
    held = [(0, np.zeros(1324, np.int8))]
    for k in range(n):
        s = slots[k]
        s["cls"] = cls[k]
        nh, h = held[-1]
        if cls[k] == FACCH9:
            m, _, _, crc, cv = orc.facch9_decode(ebits[k], ks[k])
            s["crc"], s["conv"] = (1 if crc else 0), cv
            if not crc:
                s["type"], s["len"] = 0x1a, 38
                s["l2"][:38] = m
        elif cls[k] == TCH9:
            j = t_idx.index(k)
            s["type"], s["len"], s["conv"] = 0x18, TCH9_BYTES[mode], conv[j]
            s["l2"][:TCH9_BYTES[mode]] = l2[j]
            h = np.concatenate([taken_in(ebits[k], ks[k]), h[:662]])
            nh = min(nh + 1, 2)
        held.append((nh, h))
    return slots, held


def state_of(pkg, kc, active, held):
    st = np.zeros(1, pkg.api.TCH9_STATE)
    st["active"], st["n_held"], st["kc"][0], st["held"][0] = active, held[0], kc, held[1]
    return st


@functools.lru_cache(maxsize=None)
def batch(pkg, orc, mode):
    """The five calls of BATCH_KINDS in `mode` -> dict(calls, first, ebits, sync_id, rv, fn, state): the bits form's arguments"""
    rng = np.random.default_rng(9000 + mode)
    calls = [make_call(orc, rng, kinds, mode) for kinds in BATCH_KINDS]
    first = np.concatenate([[0], np.cumsum([len(k) for k in BATCH_KINDS])]).astype(np.int32)
    state = np.concatenate([fresh_state(pkg, c["kc"]) for c in calls])
    # the call without frames holds anything at all; the last one is not active, whatever else it holds
    junk = np.frombuffer(rng.integers(0, 256, 2 * pkg.api.TCH9_STATE.itemsize, dtype=np.uint8).tobytes(), pkg.api.TCH9_STATE)
    state[1] = junk[0]
    state[4] = junk[1]
    state["active"][4] = 0
    cat = lambda f, dt: np.concatenate([np.asarray(c[f], dt).reshape((len(c["fn"]),) + np.shape(c[f])[1:]) for c in calls])
    return dict(calls=calls, first=first, ebits=cat("ebits", np.int8), sync_id=cat("sync_id", np.int32), rv=cat("rv", np.int32),
                fn=cat("fn", np.uint32), state=state)


def batch_expected(pkg, orc, mode):
    """-> (TCH9_FRAME per frame of the batch, the five states afterwards), in the decoder mode the oracle is in"""
    b = batch(pkg, orc, mode)
    slots, states = [], b["state"].copy()
    for c, call in enumerate(b["calls"]):
        n = len(call["fn"])
        if not b["state"]["active"][c]:
            off = np.zeros(n, pkg.api.TCH9_FRAME)
            off["fn"] = call["fn"]
            slots.append(off)
            continue
        if not n:
            continue
        sl, held = expected_run(pkg, orc, mode, [call["kc"]] * n, call["ebits"], call["sync_id"], call["rv"], call["fn"])
        slots.append(sl)
        states[c] = state_of(pkg, call["kc"], 1, held[-1])[0]
    return np.concatenate(slots), states


# ---- carriers for the from-samples form ----
# (sps, seed, frames): seeds chosen ON THE ORACLE ALONE so that every frame meets `carrier_margin_ok` (see there); the three sps
# pick k_rx<32,4>, k_rx<16,0> with a burst longer than 256 symbols, and k_rx<64,0>
CARRIERS = {4: [(4, 1, 21), (4, 4, 21)], 2: [(2, 5, 22), (2, 9, 20)], 11: [(11, 13, 21), (11, 14, 22)]}
CFO_HZ = 35.0


def in_len(sps):
    return 351 * sps + sps + sps // 2


@functools.lru_cache(maxsize=None)
def carrier(pkg, orc, sps, seed, n_frames, tn=5, esn0_db=28.0):
    """A CSD carrier: per frame a TCH9 burst (sync sequence 1), a burst sent with sync sequence 0 (a FACCH9) or nothing, all
    A5/1-ciphered, with a carrier frequency offset -> dict(x, kc, offset, fn, freq_shift, sent)"""
    synth = pkg.synth
    rng = np.random.default_rng(9100 + 97 * sps + seed)
    frame_len = 24 * 39 * sps
    t0 = int(rng.integers(2 * sps, frame_len // 2))
    n = t0 + (n_frames + 1) * frame_len
    fn0 = int(rng.integers(0, 1 << 18))
    kc = rng.integers(0, 256, 8, dtype=np.uint8)
    f9 = pkg.api.burst_format("nt9")
    sigma = np.sqrt(10.0 ** (-esn0_db / 10.0) / 2.0)
    x = (rng.standard_normal((n, 2)) * sigma).astype(np.float32).view(np.complex64).reshape(-1)
    il = orc.Interleaver()
    orc.lib().orc_interleaver_init(orc.C.byref(il), orc.C.c_int(3), orc.C.c_int(648))
    span, sent = 5, []
    for k in range(n_frames):
        u = rng.random()
        kind = "idle" if u < 0.12 else "facch9" if u < 0.3 else "tch9"
        sent.append(kind)
        if kind == "idle":
            continue
        ciph = orc.a5(1, kc, fn0 + k, 658)[0]
        sacch, status = rng.integers(0, 2, 10, dtype=np.uint8), rng.integers(0, 2, 4, dtype=np.uint8)
        if kind == "facch9":
            l2 = rng.integers(0, 256, 38, dtype=np.uint8)
            l2[37] &= 0x0F
            e = orc.facch9_encode(l2, sacch, status, ciph)
        else:
            l2 = rng.integers(0, 256, 60, dtype=np.uint8)
            e = np.zeros(662, np.uint8)
            orc.lib().orc_tch9_encode(e.ctypes.data_as(orc.C.c_void_p), l2.ctypes.data_as(orc.C.c_void_p), orc.C.c_int(2),
                                      sacch.ctypes.data_as(orc.C.c_void_p), status.ctypes.data_as(orc.C.c_void_p),
                                      ciph.ctypes.data_as(orc.C.c_void_p), orc.C.byref(il))
        # (below sps 4 the bursts sit 0.6 samples late: the rule of carrier_margin_ok keeps toa away from x.1 there)
        body = synth.shape_bursts(synth.map_symbols(f9, e[None, :], sync_id=0 if kind == "facch9" else 1), sps,
                                  0.6 if sps < 4 else 0.0, span)[0]
        pos = t0 + k * frame_len + tn * 39 * sps - span * sps
        x[pos:pos + body.size] += body
    ph = (2 * np.pi * CFO_HZ / (SYM_RATE * sps)) * np.arange(n, dtype=np.float64)
    x = (x * np.exp(1j * ph)).astype(np.complex64)
    e_toa = (sps + sps // 2) >> 1
    offset = np.array([t0 + k * frame_len + tn * 39 * sps - e_toa for k in range(n_frames)], np.uint64)
    assert int(offset[-1]) + in_len(sps) <= n
    return dict(sps=sps, x=x, kc=kc, offset=offset, fn=np.arange(fn0, fn0 + n_frames, dtype=np.uint32),
                freq_shift=np.full(n_frames, -2.0 * np.pi * CFO_HZ / SYM_RATE, np.float32), sent=sent)


@functools.lru_cache(maxsize=None)
def carrier_demod(pkg, orc, sps, seed, n_frames):
    """The oracle's demodulation of every frame, and of every frame with freq_shift +- 1e-5 -> list of (base, minus, plus)"""
    car = carrier(pkg, orc, sps, seed, n_frames)
    out = []
    for off, fs in zip(car["offset"], car["freq_shift"]):
        w = car["x"][int(off):int(off) + in_len(sps)]
        out.append(tuple(orc.demod("nt9", w, sps, float(fs) + d) for d in (0.0, -1e-5, 1e-5)))
    return out


def carrier_margin_ok(sps, dem):
    """The precondition under which product and oracle must agree on EVERY frame (the demod grid's rule): the oracle's rv is 0;
    its toa is more than 32/1024 from the nearest x.5 and, below sps 4, | |toa - round(toa)| - 0.1 | > 32/1024; sync_id and
    round(toa) do not move with freq_shift +- 1e-5.  -> list of the frames that miss it"""
    bad = []
    for k, (b, m, p) in enumerate(dem):
        toa = float(b["toa"])
        frac = abs(toa - np.floor(toa) - 0.5)
        ok = b["rv"] == 0 and frac > 32 / 1024
        if sps < 4:
            ok = ok and abs(abs(toa - round(toa)) - 0.1) > 32 / 1024
        ok = ok and all(o["rv"] == 0 and o["sync_id"] == b["sync_id"] and round(float(o["toa"])) == round(toa) for o in (m, p))
        if not ok:
            bad.append(k)
    return bad


# ---- the entries' argument checks ----
def bits_args(api):
    """A well-formed one-call, two-frame invocation of the bits form over host arrays (out filled with 0x55)"""
    return dict(first=np.array([0, 2], np.int32), ebits=np.zeros((2, 662), np.int8), sid=np.ones(2, np.int32),
                rv=np.zeros(2, np.int32), fn=np.arange(2, dtype=np.uint32), state=np.zeros(1, api.TCH9_STATE),
                out=np.full(160, 0x55, np.uint8).view(api.TCH9_FRAME))


def bits_bad_cases(a):
    p = lambda k: a[k].ctypes.data
    good = dict(n_calls=1, mode=2, first=p("first"), n_frames=2, ebits=p("ebits"), sid=p("sid"), rv=p("rv"), fn=p("fn"),
                state=p("state"), out=p("out"))
    bad = [dict(n_calls=-1), dict(n_frames=-1), dict(mode=-1), dict(mode=3), dict(first=None), dict(ebits=None), dict(sid=None),
           dict(fn=None), dict(state=None), dict(out=None)]
    return good, bad


def samples_args(api):
    return dict(iq=np.zeros(4096, np.complex64), first=np.array([0, 2], np.int32), off=np.array([0, 1000], np.uint64),
                fs=np.zeros(2, np.float32), fn=np.arange(2, dtype=np.uint32), state=np.zeros(1, api.TCH9_STATE),
                out=np.full(160, 0x55, np.uint8).view(api.TCH9_FRAME))


def samples_bad_cases(a):
    p = lambda k: a[k].ctypes.data
    good = dict(n_calls=1, sps=4, in_len=1410, mode=2, iq=p("iq"), iq_len=4096, first=p("first"), n_frames=2, off=p("off"),
                fs=p("fs"), fn=p("fn"), state=p("state"), out=p("out"))
    bad = [dict(sps=0), dict(sps=17), dict(in_len=1403), dict(in_len=4097), dict(mode=-1), dict(mode=3), dict(n_calls=-1),
           dict(n_frames=-1), dict(iq=None), dict(first=None), dict(off=None), dict(fs=None), dict(fn=None), dict(state=None),
           dict(out=None), dict(iq=p("iq") + 4)]
    return good, bad
