"""Aimed inputs for gmr1_fcch_rough_multi / _peak_record (reference src/sdr/fcch.c:264-496) and a float64 restatement of
the function that also says WHY a window gives the list it gives.  Shared by tests/test_fcch_multi_host.py (oracle against
this restatement, on the CPU, with the coverage of every aimed case asserted from the trace) and
tests/test_gpu_fcch_multi.py (k_fcch_multi against the oracle).

A window is low noise plus periodic dual-chirp trains.  A train at lag L (symbols) puts a correlation peak at lag L whose
flagged run is about three lags wide, so the lag aims a run of threshold flags at a bit of k_fcch_multi's flag words to
within one lag, and the amplitudes decide the order and the branch of _peak_record every rising edge takes.

The restatement is written from the reference's text in numpy; nothing is shared with the oracle's C.  Everything is
float64 except what the reference specifies in float32 and then rounds to an integer grid of its own: the phases
(freq_shift * i, the chirp's phase_base * pos^2) and the sum `i + p_fpos`, whose float32 ulp at lags of some thousands
(2^-11) is far coarser than any error of p_fpos.  With dt=np.float32 the same text runs in float32 and accumulates one
term after the other, as the reference's loops do: that form only serves to MEASURE how far float32 moves the values
the decisions hang on (measure(), below).

    python tests/fcch_multi_cases.py            prints the coverage and margins of every case and the measured figures
"""
import functools

import numpy as np

import acq_cases as ac
from f64_fcch import F32, SYM_RATE, TYPES, _c_round, _chirp_phase

PERIOD = (320 * SYM_RATE) // 1000          # 7488 symbols
N_SYM = 15400                              # default window: every lag below Lw + 7498 is inside the sweep (117-symbol burst)
N_SYM3 = 16000                             # the same for the 468-symbol burst
EINVAL = -22

# ---------------------------------------------------------------------------------------------------------------------
# margins.  The outputs are integers and are compared for equality, which is fair only where no rounding of float32
# against float32 (the oracle's sums in the reference's order, the kernel's in its own) can flip a decision.  measure()
# ran every case below through the restatement in float32 (sequential sums) and in float64 and took the largest distance
# between the two runs; every margin has to be 50 times the measured figure of its kind:
#   REL   relative: mixed values and threshold (in units of the threshold), peak powers, the strongest lag's lead
#   FPOS  symbols: p_fpos; the position adds one ulp of the float32 sum `i + p_fpos` at lags below 8192, since a
#         difference in p_fpos however small may move that sum by one ulp
#   DLP   lags: peaks[1] - peaks[0], whose float32 centroids of lags near 15 000 carry ulps of 2^-10 themselves
# (measured by `python tests/fcch_multi_cases.py`, figures rounded up; tests/test_fcch_multi_host.py re-measures and
# fails if a case added later moves further than these)
# ---------------------------------------------------------------------------------------------------------------------
REL_MEASURED = 7e-5
FPOS_MEASURED = 3e-7
DLP_MEASURED = 4e-3
FACTOR = 50
REL_MARGIN = FACTOR * REL_MEASURED
FPOS_MARGIN = FACTOR * FPOS_MEASURED + 2.0 ** -11
DLP_MARGIN = FACTOR * DLP_MEASURED


def min_len(sps):
    return (650 * SYM_RATE * sps) // 1000


# ---------------------------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------------------------
def make_window(pkg, which, sps, n, trains, period=PERIOD, seed=0, noise=0.05, cfo=0.0, loud=()):
    """n samples: complex Gaussian noise of standard deviation `noise` plus, per train (lag in symbols, amplitude
    [, gains]), synth.fcch_dual_chirp copies every `period` symbols from the lag on.  gains: factors on the successive
    copies (the last one holds for all later copies; a 0 ends the train).  A copy that does not fit is cut off at the
    window's end.  cfo: carrier offset in rad / symbol.  loud: (first symbol, symbols) stretches whose noise has standard
    deviation 1."""
    freq, blen = TYPES[which]
    rng = np.random.default_rng([4021, seed])
    g = rng.standard_normal((n, 2)) * (noise / np.sqrt(2.0))
    x = g[:, 0] + 1j * g[:, 1]
    for a, m in loud:
        x[a * sps:(a + m) * sps] *= 1.0 / noise
    chirp = pkg.synth.fcch_dual_chirp(freq, blen, sps).astype(np.float64)
    for tr in trains:
        lag, amp = tr[0], tr[1]
        gains = tr[2] if len(tr) > 2 else (1.0,)
        pos, k = int(round(lag * sps)), 0
        while pos < n:
            gk = gains[min(k, len(gains) - 1)]
            if gk == 0.0:
                break
            m = min(chirp.size, n - pos)
            x[pos:pos + m] += (amp * gk) * chirp[:m]
            pos += period * sps
            k += 1
    if cfo:
        x = x * np.exp(1j * cfo * np.arange(n) / sps)
    return x.astype(np.complex64)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _seq_sum(a, dt):
    """float32: one term after the other (cumsum does not sum pairwise), as the reference's loops"""
    return np.cumsum(a)[-1] if dt is np.float32 else a.sum()


def _half_dist(v):
    """distance of v from the nearest point where round() changes"""
    return abs(abs(v - np.floor(v)) - 0.5)


def _rel(a, b):
    return abs(float(a) - float(b)) / max(float(a), float(b))


def _record(toa, pwr, n, N, Lp, sps, half, p_toa, p_pwr, ev, cmps):
    """_peak_record (fcch.c:264-326) -> the new count; ev gets the branch taken, cmps every pair of powers compared"""
    has_dupe = 0
    i = 0
    while i < n:
        d = (toa[i] % Lp) - (p_toa % Lp)            # samples modulo a period in SYMBOLS: the reference's text
        if abs(d) > half:
            i += 1
            continue
        # a duplicate by that rule; an aliased one if the two are not within half a burst modulo the period in samples
        t = (toa[i] - p_toa) % (Lp * sps)
        if min(t, Lp * sps - t) > half:
            ev["aliased"] = True
        cmps.append(_rel(pwr[i], p_pwr))
        if pwr[i] > p_pwr:
            if not has_dupe:
                has_dupe = 1
            i += 1
            continue
        for j in range(i, n - 1):
            toa[j], pwr[j] = toa[j + 1], pwr[j + 1]
        n -= 1
        has_dupe = -1
        ev["removed"] += 1
        i += 1                                       # (the entry that moved into slot i is not looked at: as the reference)
    if has_dupe > 0:
        ev["blocked"] = True
        return n
    i = 0
    while i < n:
        cmps.append(_rel(p_pwr, pwr[i]))
        if p_pwr > pwr[i]:
            break
        i += 1
    if i == N:
        ev["gave_up"] = True
        return n
    if n == N:
        ev["dropped_last"] = True
    for j in range(N - 1, i, -1):
        toa[j], pwr[j] = toa[j - 1], pwr[j - 1]
    toa[i], pwr[i] = p_toa, p_pwr
    ev["inserted"] = True
    return n if n == N else n + 1


def _peak_at(v, i, sps):
    """fcch.c:469-472 -> (p_pwr, p_fpos, i + p_fpos as the float32 the reference forms, p_pos)"""
    p_pwr = v[i - 1] + v[i] + v[i + 1]
    fpos = (-v[i - 1] + v[i + 1]) / p_pwr
    xs = F32(F32(i) + F32(fpos))                                          # float32 by specification (see the module's text)
    return p_pwr, fpos, xs, _c_round(float(F32(xs * F32(sps))))


def model(x, sps, freq_shift=0.0, N=16, which="fcch", dt=np.float64):
    """gmr1_fcch_rough_multi -> (count or -22, list of toa, trace).  trace: i0, nLp, d (peaks[1] - peaks[0]), nlags,
    past_end (lags below Lw whose partner lies beyond the sweep), overread (the partner lies beyond the zeros the oracle
    keeps behind its sweep: the reference's own answer is then undefined), runs [(first, last)], events (one dict per
    rising edge), margins dict(thr, pos, dlp, pwr, lead), and the values measure() compares (v, th, fpos, pwrs)."""
    T = dt
    ct = np.complex64 if dt is np.float32 else np.complex128
    freq, blen = TYPES[which]
    tr = dict(margins={})
    if len(x) < min_len(sps):
        return EINVAL, [], tr
    # osmo_cxvec_sig_normalize: statistics over every raw sample, then decimation and rotation
    X = np.asarray(x).astype(ct)
    nraw = T(X.size)
    avg = _seq_sum(X, dt) / nraw
    dX = X - avg
    sd = np.sqrt(_seq_sum(dX.real * dX.real + dX.imag * dX.imag, dt) / nraw)
    if sd == 0:
        sd = T(1.0)
    ln = X.size // sps
    w = (X[::sps][:ln] - avg) / sd
    fs = F32(freq_shift)
    if fs != F32(0.0):
        ph = (fs * np.arange(ln, dtype=F32)).astype(dt)                   # the float32 product is the specification
        w = w * (np.cos(ph) + 1j * np.sin(ph)).astype(ct)
    ref = (T(np.sqrt(T(2.0))) * np.cos(_chirp_phase(freq, blen).astype(dt))).astype(dt)
    cl = ln - blen + 1
    if dt is np.float32:
        acc = np.zeros(cl, ct)
        for k in range(blen):
            acc += ref[k] * w[k:k + cl]
        e = acc.real * acc.real + acc.imag * acc.imag
    else:
        re, im = np.correlate(w.real, ref, "valid"), np.correlate(w.imag, ref, "valid")
        e = re * re + im * im
    Lw, Lp = PERIOD + blen, PERIOD
    cp = np.zeros(max(cl, Lw + PERIOD + 11) + 64, dt)                     # lags beyond the sweep count as 0
    cp[:cl] = e
    # strongest lag of the first Lw: the first maximum, and it has to exceed 0
    head = cp[:min(Lw, cl)]
    i0 = int(np.argmax(head)) if head.max() > 0 else 0
    rest = np.delete(head, i0)
    tr.update(i0=i0, nlags=cl, lead=float((head[i0] - rest.max()) / head[i0]) if head[i0] > 0 else 0.0)
    pw, pk = [T(0.0), T(0.0)], [T(0.0), T(0.0)]
    for k in range(-10, 11):
        for h, j in enumerate((i0 + k, i0 + k + Lp)):
            if 0 < j < cl:
                pw[h] = pw[h] + cp[j]
                pk[h] = pk[h] + cp[j] * T(j)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = pk[1] / pw[1] - pk[0] / pw[0]
    if not np.isfinite(d):
        tr.update(nLp=None, d=None)
        return EINVAL, [], tr                                             # (int)round(NaN): |nLp - Lp| > 10 on every platform here
    nLp = _c_round(float(d))
    tr.update(nLp=nLp, d=float(d))
    tr["margins"]["dlp"] = float(_half_dist(float(d)))
    tr["margins"]["lead"] = tr["lead"]
    if abs(nLp - Lp) > 10:
        return EINVAL, [], tr
    Lp = nLp
    tr.update(past_end=max(0, Lw + Lp - cl), overread=Lw + Lp > cl + 64)
    # the two cycles mixed, mean, deviation, threshold
    v = np.sqrt(cp[:Lw] * cp[Lp:Lp + Lw])
    avg = _seq_sum(v, dt) / T(Lw)
    dv = v - avg
    th = avg + T(3.0) * np.sqrt(_seq_sum(dv * dv, dt) / T(Lw))
    flags = v > th
    flags[0] = flags[Lw - 1] = False                                      # for (i=1; i<Lw-1; i++)
    tr.update(v=v, th=float(th))
    tr["margins"]["thr"] = float(np.min(np.abs(v[1:Lw - 1] - th)) / th) if th > 0 else 0.0
    edge = flags & ~np.concatenate([[False], flags[:-1]])
    fall = flags & ~np.concatenate([flags[1:], [False]])
    tr["runs"] = list(zip(np.flatnonzero(edge).tolist(), np.flatnonzero(fall).tolist()))
    half = (blen * sps) >> 1
    toa, pwr, n = [0] * N, [T(0.0)] * N, 0
    events, cmps, pos_m, fposs, pwrs = [], [], [], [], []
    for i in np.flatnonzero(edge).tolist():
        p_pwr, fpos, xs, p_pos = _peak_at(v, i, sps)
        pos_m.append(float(_half_dist(float(xs) * sps)) / sps)
        fposs.append(float(fpos))
        pwrs.append(float(p_pwr))
        ev = dict(lag=i, pos=p_pos, pwr=float(p_pwr), n_before=n, removed=0, blocked=False, gave_up=False, inserted=False,
                  dropped_last=False, aliased=False)
        n = _record(toa, pwr, n, N, Lp, sps, half, p_pos, p_pwr, ev, cmps)
        events.append(ev)
    tr.update(events=events, fpos=fposs, pwrs=pwrs)
    tr["margins"]["pos"] = min(pos_m) if pos_m else 1.0
    tr["margins"]["pwr"] = min(cmps) if cmps else 1.0
    return n, toa[:n], tr


# ---------------------------------------------------------------------------------------------------------------------
# k_fcch_multi's ordered tail with a slip in it.  Nothing above depends on this: it replays a finished trace (mixed values,
# threshold, measured period) the way the KERNEL walks it -- flag words of 32 lags, a carry bit between them, a third list
# s_mod[] of toa % Lp next to toa[] and pwr[] -- so that the windows which would notice a slip can be named.
# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("no_before", "short_word", "q_lt_n", "mod_not_shifted", "mod_in_symbols")


def slipped(count, tr, sps, N, which, mut):
    """-> (count, list) k_fcch_multi would return for the window of trace tr with `mut` built in: the carry bit between
    two flag words dropped; the last, partial flag word left out; `q != N` written as `q < n`; s_mod[] left behind when
    toa[] and pwr[] shift; the new peak's modulus taken in symbols.  mut=None: the kernel as it is."""
    if count < 0:
        return count, []
    v, Lp = tr["v"], tr["nLp"]
    Lw = len(v)
    flags = v > tr["th"]
    flags[0] = flags[Lw - 1] = False
    below = np.concatenate([[False], flags[:-1]])
    if mut == "no_before":
        below[::32] = False
    edge = flags & ~below
    if mut == "short_word":
        edge = edge & ((np.arange(Lw) // 32 + 1) * 32 < Lw)
    half = (TYPES[which][1] * sps) >> 1
    toa, pwr, mod, n = [0] * N, [0.0] * N, [0] * N, 0
    for i in np.flatnonzero(edge).tolist():
        p_pwr, _, _, p_pos = _peak_at(v, i, sps)
        p_mod = (p_pos // sps) % Lp if mut == "mod_in_symbols" else p_pos % Lp
        has_dupe, q = 0, 0
        while q < n:
            if abs(mod[q] - p_mod) > half:
                q += 1
                continue
            if pwr[q] > p_pwr:
                has_dupe = has_dupe or 1
                q += 1
                continue
            for j in range(q, n - 1):
                toa[j], pwr[j] = toa[j + 1], pwr[j + 1]
                if mut != "mod_not_shifted":
                    mod[j] = mod[j + 1]
            n -= 1
            has_dupe = -1
            q += 1
        if has_dupe > 0:
            continue
        q = 0
        while q < n and not p_pwr > pwr[q]:
            q += 1
        if (q < n) if mut == "q_lt_n" else (q != N):
            for j in range(N - 1, q, -1):
                toa[j], pwr[j] = toa[j - 1], pwr[j - 1]
                if mut != "mod_not_shifted":
                    mod[j] = mod[j - 1]
            toa[q], pwr[q], mod[q] = p_pos, p_pwr, p_mod
            if n != N:
                n += 1
    return n, toa[:n]


def margins_ok(tr):
    """-> list of the margins the trace misses (empty: no float32 rounding can decide this window)"""
    m = tr["margins"]
    need = dict(dlp=DLP_MARGIN, lead=REL_MARGIN, thr=REL_MARGIN, pos=FPOS_MARGIN, pwr=REL_MARGIN)
    return ["%s %.3g < %.3g" % (k, m[k], need[k]) for k in need if k in m and not m[k] >= need[k]]


def coverage(tr, count, N):
    """what a window reached, as a set of tags, from its trace"""
    tags = set()
    if count < 0:
        tags.add("error")
        if tr.get("nLp") is None:
            return tags
    i0, cl = tr["i0"], tr["nlags"]
    if i0 < 10:
        tags.add("i0_low")
    if i0 + PERIOD + 10 >= cl:
        tags.add("i0_high")
    if count < 0:
        return tags
    if tr["nLp"] != PERIOD:
        tags.add("period")
    if tr["past_end"]:
        tags.add("past_end")
    if count == N:
        tags.add("full")
    for ev in tr["events"]:
        for k in ("blocked", "gave_up", "inserted", "dropped_last", "aliased"):
            if ev[k]:
                tags.add(k)
        if ev["removed"]:
            tags.add("removed")
        if ev["removed"] and ev["inserted"]:
            tags.add("replaced")
    Lw = len(tr["v"])
    for a, b in tr["runs"]:
        if b % 32 == 31:
            tags.add("ends_bit31")
        if a % 32 == 0:
            tags.add("starts_bit0")
        # the coarsest boundary the run lies across: word (32 lags), wave (64), round (256), ballot (2048)
        across = [step for step in (32, 64, 256, 2048) if a // step != b // step]
        if across:
            tags.add("straddles_%d" % across[-1])
        if a // 32 == (Lw - 1) // 32:
            tags.add("last_word")
        if a // 32 > 237:
            tags.add("above_word_237")
        if a == 1:
            tags.add("starts_lag1")
        if b == Lw - 2:
            tags.add("ends_last_lag")
    return tags


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
FIVE = [(500, 1.0), (1500, 0.6), (2500, 1.4), (3500, 0.8), (4500, 1.2)]


def _forty():
    # amplitudes 0.8 ... 1.2 in shuffled order, their squares (what a peak's power follows) in equal ratios of 2 %: drawn
    # at random, two of forty powers come closer to each other than the margin on compared powers allows
    rank = np.random.default_rng(4040).permutation(40)
    return [(150 + 180 * k, float(0.8 * 1.5 ** (rank[k] / 39.0))) for k in range(40)]


def _case(name, trains, aims=(), which="fcch", sps=4, n_sym=None, n=None, N=16, period=PERIOD, seed=None, cfo=0.0,
          fs=0.0, noise=0.05, kind="trains", pad=False, count=None):
    if n_sym is None:
        n_sym = N_SYM if which == "fcch" else N_SYM3
    return dict(name=name, trains=tuple(trains), aims=frozenset(aims), which=which, sps=sps, n=n if n else n_sym * sps, N=N,
                period=period, seed=seed, cfo=cfo, fs=fs, noise=noise, kind=kind, pad=pad, count=count)


def case_list():
    """The aimed cases.  aims: the tags coverage() has to report for the case (tests/test_fcch_multi_host.py asserts
    them); count: the count the case is built for."""
    c = []
    # ---- the list's size: five trains of different strength, then forty
    c.append(_case("five_N1", FIVE, {"full", "gave_up", "dropped_last"}, N=1, seed=1, count=1))
    c.append(_case("five_N2", FIVE, {"full", "gave_up", "dropped_last"}, N=2, seed=1, count=2))
    c.append(_case("five_N3", FIVE, {"full", "dropped_last"}, N=3, seed=1, count=3))
    c.append(_case("five_N32", FIVE, {"inserted"}, N=32, seed=1))
    forty = _forty()
    c.append(_case("forty_sps1_N32", forty, {"full", "dropped_last"}, sps=1, N=32, seed=117, count=32))
    c.append(_case("forty_sps1_N16", forty, {"full", "gave_up", "dropped_last"}, sps=1, N=16, seed=117, count=16))
    c.append(_case("forty_sps1_N2", forty, {"full", "gave_up", "dropped_last"}, sps=1, N=2, seed=117, count=2))
    # ---- toa % Lp with toa in samples and Lp in symbols: trains 7488 / sps symbols apart are "duplicates"
    c.append(_case("forty_sps4_N32", forty, {"aliased", "blocked", "removed"}, sps=4, N=32, seed=101))
    c.append(_case("alias_weak_first", [(1000, 0.7), (2872, 1.0), (5000, 0.85)], {"aliased", "replaced"}, seed=4))
    c.append(_case("alias_strong_first", [(1000, 1.0), (2872, 0.7), (5000, 0.85)], {"aliased", "blocked"}, seed=5))
    # ---- a train below the burst length shows twice within Lw, one period apart
    c.append(_case("twice_blocked", [(40, 1.0, (1.2, 1.0, 0.6)), (3000, 0.8)], {"blocked"}, seed=6))
    c.append(_case("twice_replaced", [(40, 1.0, (1.0, 1.2, 1.6)), (3000, 0.8)], {"replaced"}, seed=7))
    c.append(_case("lag3", [(3, 1.2, (1.2, 1.0, 0.6)), (3000, 0.8)], {"i0_low", "blocked"}, seed=8))
    # ---- two trains within half a burst of each other
    c.append(_case("near_strong_first", [(2000, 1.0), (2030, 0.7), (5000, 0.85)], {"blocked"}, seed=9))
    c.append(_case("near_weak_first", [(2000, 0.7), (2030, 1.0), (5000, 0.85)], {"replaced"}, seed=100))
    # ---- runs of flags on the boundaries of k_fcch_multi's words, waves, rounds and ballots
    c.append(_case("bounds_word", [(1598, 1.0), (2273, 0.8), (2912, 1.2), (3392, 0.9), (4864, 1.1)],
                   {"ends_bit31", "starts_bit0", "straddles_32", "straddles_64", "straddles_256"}, seed=11))
    c.append(_case("bounds_2048", [(2047, 1.0), (4095, 0.8), (6143, 1.2)], {"straddles_2048"}, seed=12))
    c.append(_case("bounds_ends", [(1, 1.4, (1.2, 1.0, 0.6)), (7590, 0.8), (3000, 1.2)], {"starts_lag1", "last_word", "i0_low"},
                   seed=13))
    c.append(_case("bounds_last_lag", [(7603, 1.0), (3000, 0.8)], {"ends_last_lag", "last_word"}, seed=14))
    # ---- the shortest window there is: the strongest lag's twin lies at the end of the sweep or beyond it
    # (lag 100: the twin's centroid still ends inside the sweep, the control of the other two)
    for lag in (100, 112, 116):
        c.append(_case("min_len_%d" % lag, [(lag, 1.0, (1.0, 1.4, 0.7)), (3000, 0.8)], {"i0_high"} if lag > 100 else (),
                       n=min_len(4), seed=15 + lag))
    # (and with a longer period the last lags below Lw are paired with lags beyond the sweep: they count as 0)
    c.append(_case("min_len_period_7494", [(700, 1.0), (4100, 0.8)], {"period", "past_end"}, n=min_len(4), period=7494, seed=100))
    # ---- the measured period
    for per in (7485, 7491, 7498):
        c.append(_case("period_%d" % per, [(700, 1.0), (4100, 0.8)], {"period"}, period=per, seed=20 + per % 10))
    # ---- samples per symbol, carrier offset
    mixed = [(321.5, 1.0), (1777.25, 0.7), (4000.75, 1.3), (6500, 0.85)]
    for sps in (1, 2, 8, 16):
        c.append(_case("mixed_sps%d" % sps, mixed, {"inserted"}, sps=sps, seed=30 + sps))
    c.append(_case("carrier_offset", mixed, {"inserted"}, cfo=0.03, fs=-0.03, seed=40))
    # ---- the 468-symbol burst: Lw = 7956, flag words up to 248
    c.append(_case("fcch3_650ms", [(200, 1.0), (1500, 0.7), (3100, 1.3)], {"inserted", "past_end"}, which="fcch3_lband",
                   n=min_len(4), pad=True, seed=41))
    c.append(_case("fcch3_long", [(300, 1.0), (2500, 0.7), (5200, 1.3), (7000, 0.85)], {"inserted"}, which="fcch3_lband", seed=104))
    c.append(_case("fcch3_word_245", [(7840, 1.0), (2500, 0.8), (5200, 1.2)], {"above_word_237", "straddles_32"},
                   which="fcch3_lband", seed=43))
    # ---- no answer
    c.append(_case("zeros", [], {"error"}, n=min_len(4), kind="zeros", count=EINVAL))
    c.append(_case("constant", [], {"error"}, n=min_len(4), kind="constant", count=EINVAL))
    c.append(_case("lone_burst", [(1000, 1.0, (1.0, 0.0))], seed=100))
    # (noise all over the window flags a hundred runs and leaves some of 7605 values within a thousandth of the threshold
    # whatever the seed: no margin can hold there -- tests/test_gpu_fcch.py has that window, unguarded.  Here the noise is
    # loud over 400 symbols and once more a period later, so that a dozen runs come out of noise alone)
    c.append(_case("noise", [], kind="noise_bursts", seed=222))
    return c


@functools.lru_cache(maxsize=None)
def _window_of(pkg, key):
    which, sps, n, trains, period, seed, noise, cfo, kind = key
    if kind == "zeros":
        return np.zeros(n, np.complex64)
    if kind == "constant":
        return np.full(n, 0.5 - 0.25j, np.complex64)       # (every partial sum of it is exact in float32: the mean leaves 0)
    loud = ((1000, 400), (1000 + PERIOD, 400)) if kind == "noise_bursts" else ()
    return make_window(pkg, which, sps, n, trains, period, seed, noise, cfo, loud)


def window(pkg, c):
    """the case's samples (built once; cases that differ in N only share them) -- read-only"""
    x = _window_of(pkg, (c["which"], c["sps"], c["n"], c["trains"], c["period"], c["seed"], c["noise"], c["cfo"], c["kind"]))
    x.setflags(write=False)
    return x


def oracle_window(pkg, c):
    """what the oracle and the restatement are given: the window, for the 650 ms FCCH3 case with acq_cases.multi_window's
    zeros behind it (the reference reads past its sweep there)"""
    x = window(pkg, c)
    return ac.multi_window(x, c["sps"], c["which"]) if c["pad"] else x


_results = {}


def expected(pkg, orc, c):
    """-> (count, list) from the oracle, computed once per case"""
    if c["name"] not in _results:
        cnt, toa = orc.fcch_rough_multi(oracle_window(pkg, c), c["sps"], c["fs"], c["N"], c["which"])
        _results[c["name"]] = (int(cnt), [int(t) for t in toa])
    return _results[c["name"]]


# ---------------------------------------------------------------------------------------------------------------------
# carriers for the batched acquisition (gmr1_hip_fcch_acquire_batch), held to acq_cases.expected
# ---------------------------------------------------------------------------------------------------------------------
def acq_carriers(pkg):
    """[(name, samples, start)]: 1.5 s at 4 samples a symbol.  `crowded`: twenty trains, so that rough_multi hands step 3
    a full list of sixteen (and drops the last entry on the way); `aliased`: two trains 1872 symbols apart, which _peak_record takes for one."""
    n = ac.N_15
    # (281 symbols apart: no two of the twenty come within half a burst of each other modulo 7488 / 4 symbols, so none is
    # another's aliased duplicate; amplitudes 0.9 ... 1.1 shuffled, their squares in equal ratios of 2 %)
    rank = np.random.default_rng(4041).permutation(20)
    crowded = [(2100 + 281 * k, float(0.9 * (1.1 / 0.9) ** (rank[k] / 19.0))) for k in range(20)]
    return [("crowded", make_window(pkg, "fcch", ac.SPS, n, crowded, seed=50), 8000),
            ("aliased", make_window(pkg, "fcch", ac.SPS, n, [(2500, 1.0), (4372, 0.8), (6000, 0.9)], seed=51), 8000)]


# ---------------------------------------------------------------------------------------------------------------------
# the measurement behind the margins
# ---------------------------------------------------------------------------------------------------------------------
def measure(pkg, cases=None):
    """-> dict(rel, fpos, dlp, worst): the largest distance between the float32 (sequential) and the float64 run of the
    restatement over the cases, per kind of value"""
    out = dict(rel=0.0, fpos=0.0, dlp=0.0, raw=0.0)
    worst = {}
    seen = set()
    for c in cases or case_list():
        key = (c["which"], c["sps"], c["n"], c["trains"], c["period"], c["seed"], c["noise"], c["cfo"], c["kind"], c["fs"])
        if key in seen:
            continue
        seen.add(key)
        x = oracle_window(pkg, c)
        r64 = model(x, c["sps"], c["fs"], 32, c["which"], np.float64)
        r32 = model(x, c["sps"], c["fs"], 32, c["which"], np.float32)
        t64, t32 = r64[2], r32[2]
        if t64.get("d") is None or "v" not in t64 or "v" not in t32:
            continue
        got = dict(dlp=abs(t64["d"] - t32["d"]), rel=0.0, fpos=0.0, raw=0.0)
        th, th32 = t64["th"], t32["th"]
        v32 = t32["v"].astype(np.float64)
        got["raw"] = max(float(np.max(np.abs(t64["v"] - v32))) / th, abs(th - th32) / th)
        # (in units of each run's own threshold: a factor common to all values of a run decides nothing)
        u64, u32 = t64["v"] / th, v32 / th32
        got["rel"] = float(np.max(np.abs(u64 - u32) / np.maximum(u64, 1.0)))
        if [e["lag"] for e in t64["events"]] == [e["lag"] for e in t32["events"]]:
            for a, b in zip(t64["pwrs"], t32["pwrs"]):
                got["raw"] = max(got["raw"], abs(a - b) / a)
                got["rel"] = max(got["rel"], abs(a / th - b / th32) / (a / th))
            for a, b in zip(t64["fpos"], t32["fpos"]):
                got["fpos"] = max(got["fpos"], abs(a - b))
        for k in out:
            if got[k] > out[k]:
                out[k], worst[k] = got[k], c["name"]
    out["worst"] = worst
    return out


if __name__ == "__main__":
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from __graft_entry__ import load_package
    import oracle_lib
    oracle_lib.build()
    pkg = load_package()
    t0 = time.time()
    for c in case_list():
        cnt, toa, tr = model(oracle_window(pkg, c), c["sps"], c["fs"], c["N"], c["which"])
        o = expected(pkg, oracle_lib, c)
        tags = coverage(tr, cnt, c["N"])
        print("%-20s model %3d oracle %3d %s i0 %s nLp %s d %s runs %d missing %s margins %s %s" % (
            c["name"], cnt, o[0], "same" if (cnt, toa) == o else "DIFFERENT", tr.get("i0"), tr.get("nLp"),
            None if tr.get("d") is None else round(tr["d"], 3), len(tr.get("runs", [])),
            sorted(c["aims"] - tags), {k: float("%.3g" % v) for k, v in tr["margins"].items()},
            margins_ok(tr) if "pos" in tr["margins"] else ""))
        if "-v" in sys.argv:
            print("    runs", tr.get("runs"))
            for ev in tr.get("events", []):
                print("   ", {k: v for k, v in ev.items() if v or k == "lag"})
    print("%.1f s" % (time.time() - t0))
    t0 = time.time()
    print("measured", measure(pkg), "%.1f s" % (time.time() - t0))
