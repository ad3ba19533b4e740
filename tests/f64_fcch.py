"""float64 restatement of the reference's fine FCCH acquisition and FCCH SNR estimate (gmr1_fcch_fine / gmr1_fcch_snr,
reference src/sdr/fcch.c:512-708), and the case grid that tests/test_fcch_f64_host.py (oracle against this restatement, on
the CPU) and tests/test_gpu_fcch_fine_grid.py (product against oracle) share.

Written from the reference's text, in numpy, with the DFT by FFT: nothing here is shared with the oracle's C.  Everything is
float64 except what the reference *specifies* in float32: the phases are fp32 products there (freq_shift * i, the chirp's
phase_base * pos^2, the half-band shift's 2 pi mid / len * i), and a phase of a thousand radians rounded to fp32 is a
different angle from the exact product, so the rounded product is part of what is computed, not an error of it.  The
sines and cosines of those phases, the statistics, the products, the DFT and the centroids are all float64.

The restatement returns more than the answers: the continuous toa_samples (before the reference rounds it), and the
relative energy margin of the best 5-bin window over the best window that does not overlap it.  A case whose margin is
below MARGIN_MIN, or whose toa_samples lies within HALF_DELTA of a half-integer, is one that fp32 rounding may decide
either way: the grid tests leave its toa out (at most 2 % of any cell) and say so.

    python tests/f64_fcch.py --sweep [N]     measures HALF_DELTA (see measure_half_delta)
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F32 = np.float32
SYM_RATE = 23400
TYPES = {"fcch": (0.32, 117), "fcch3_lband": (0.32, 468), "fcch3_sband": (0.16, 468)}

# product against oracle
TOL_FREQ = 1e-4          # rad / symbol
TOL_SNR = 2e-4           # relative (of max(1, |snr|))
MARGIN_MIN = 1e-3        # the figure tests/test_gpu_fcch_fold.py uses for a window that leads by too little
# Four times the measured figure.  measure_half_delta(seed=20261, n_random=20000) -- 20 000 random bursts over the whole
# grid plus 400 bursts steered onto a half-integer and stepped across it -- saw the oracle and this restatement round to
# different integers at distances from the half-integer of up to HALF_DELTA_MEASURED samples, and never further out.
HALF_DELTA_MEASURED = 6.352e-4     # samples: 866 disagreements in 28 820 bursts compared, none further out
HALF_DELTA = 4 * HALF_DELTA_MEASURED


def _chirp_phase(freq, n):
    """fcch.c:92-121 at sps = 1, the phase as the reference forms it: fp32 throughout."""
    phase_base = F32(F32(F32(freq) * F32(2.0)) * F32(np.pi)) / F32(n)
    pos = np.arange(n, dtype=F32) - F32(n) / F32(2.0)
    return (phase_base * (pos * pos)).astype(np.float64)


def _normalised(x, sps, n, freq_shift):
    """osmo_cxvec_sig_normalize: statistics over all raw samples, decimation, rotation by freq_shift per symbol."""
    x = np.asarray(x).astype(np.complex128)
    avg = x.mean()
    sd = np.sqrt(np.mean(np.abs(x - avg) ** 2))
    if sd == 0.0:
        sd = 1.0
    b = (x[::sps][:n] - avg) / sd
    fs = F32(0.0 if freq_shift is None else freq_shift)
    if fs != F32(0.0):
        ph = (fs * np.arange(n, dtype=F32)).astype(np.float64)        # the fp32 product is the specification
        b = b * np.exp(1j * ph)
    return b


def _c_round(v):
    return int(np.sign(v) * np.floor(abs(v) + 0.5))                   # C round(): halves away from zero


def _window_peak(e):
    """PEAK_WEIGH_WIN over 5 bins: (centroid, relative margin of the best window over the best one not overlapping it)"""
    w = np.convolve(e, np.ones(5), "valid")
    mi = int(np.argmax(w))                                            # first maximum, as the reference's strict '>'
    k = np.arange(mi, mi + 5)
    den = e[k].sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = (e[k] * k).sum() / den
    other = w.copy()
    other[max(0, mi - 4):mi + 5] = -np.inf
    margin = (w[mi] - other.max()) / w[mi] if w[mi] > 0 else 0.0
    return pos, margin


def fine(x, sps, freq_shift=None, which="fcch"):
    """-> dict(rv, toa, freq_error, toa_samples, margin); toa is None where toa_samples is not a number."""
    freq, n = TYPES[which]
    if len(x) // sps != n:
        return dict(rv=-22)
    b = _normalised(x, sps, n, freq_shift)
    up = np.sqrt(0.5) * np.exp(1j * _chirp_phase(freq, n))
    mid = n >> 1
    phf = (F32(F32(F32(2.0) * F32(np.pi)) * F32(mid)) / F32(n) * np.arange(n, dtype=F32)).astype(np.float64)
    shift = np.exp(1j * phf)                                          # centres the spectrum on bin n / 2
    peaks, margins = [], []
    for ref in (up, np.conj(up)):
        spec = np.fft.fft(b * ref * shift)
        p, m = _window_peak(spec.real ** 2 + spec.imag ** 2)
        peaks.append(p)
        margins.append(m)
    bin_hz = SYM_RATE / n
    pu, pd = (peaks[0] - mid) * bin_hz, (peaks[1] - mid) * bin_hz
    freq_error = 2.0 * np.pi * ((pu + pd) / 2.0) / SYM_RATE
    chirp_rate = 2.0 * float(F32(freq)) * SYM_RATE * SYM_RATE / (n * 1000)
    toa_samples = ((pu - pd) / 2.0) / chirp_rate * SYM_RATE * sps / 1000.0
    return dict(rv=0, toa=_c_round(toa_samples) if np.isfinite(toa_samples) else None, freq_error=float(freq_error),
                toa_samples=float(toa_samples), margin=float(min(margins)))


def snr(x, sps, freq_shift=None, which="fcch"):
    """-> (rv, snr): the two largest bins of the dual-chirp product's spectrum over the fifth and sixth"""
    freq, n = TYPES[which]
    if len(x) // sps != n:
        return -22, None
    b = _normalised(x, sps, n, freq_shift) * (np.sqrt(2.0) * np.cos(_chirp_phase(freq, n)))
    spec = np.fft.fft(b)
    e = np.sort(spec.real ** 2 + spec.imag ** 2)[::-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return 0, float((e[0] + e[1]) / (e[4] + e[5]))


def undecidable(f, half_delta=None):
    """why fp32 rounding may decide this case's toa either way: "margin", "half" or None"""
    if not f["margin"] >= MARGIN_MIN:
        return "margin"
    d = HALF_DELTA if half_delta is None else half_delta
    t = f["toa_samples"]
    if abs(abs(t - np.floor(t)) - 0.5) < d:
        return "half"
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------------------------
SPS_GRID = (1, 2, 3, 4, 5, 8, 16)
SHIFT_CLASSES = ("none", "zero", "small", "loop", "edge")
SNRS_DB = (0.0, 3.0, 6.0, 10.0, 20.0, None)         # None: a noiseless burst
CELL = 50                                           # cases per cell (type x sps x shift class): 2 % of it is one case
GRID_SEED = 7118                                    # (7117 puts two cases of one cell within HALF_DELTA of a half-integer)


def body_of(which, sps):
    """which of k_fcch_fine's two bodies a window of this type and sps reaches (fcch_kernels.hip: nraw <= 512)"""
    return "registers" if TYPES[which][1] * sps <= 512 else "memory"


def make_burst(rng, which, sps, snr_db, cfo_hz, delay, dc):
    """A window of exactly len * sps samples: the dual chirp sqrt(2) cos(phi(t)) delayed by `delay` samples (a real
    number), noise of variance 1 per complex sample under it unless snr_db is None, a carrier offset, a DC offset."""
    freq, n = TYPES[which]
    k = np.arange(n * sps, dtype=np.float64)
    u = (k - delay) / sps
    chirp = np.sqrt(2.0) * np.cos(freq * 2 * np.pi / n * (u - n / 2.0) ** 2) * ((u >= 0) & (u < n))
    if snr_db is None:
        x = chirp.astype(np.complex128)
    else:
        noise = rng.standard_normal((k.size, 2))
        x = (noise[:, 0] + 1j * noise[:, 1]) / np.sqrt(2.0) + np.sqrt(10.0 ** (snr_db / 10.0)) * chirp
    x = x * np.exp(1j * (2 * np.pi * cfo_hz / (SYM_RATE * sps) * k + rng.uniform(0, 2 * np.pi))) + dc
    return x.astype(np.complex64)


def cell_cases(which, sps, cls, count=CELL, seed=GRID_SEED):
    """The cases of one grid cell, the same on every machine: list of dict(x, fs, snr_db, cfo_hz).  fs is None (no
    freq_shift array at all), or the float32 the caller passes."""
    rng = np.random.default_rng([seed, list(TYPES).index(which), sps, SHIFT_CLASSES.index(cls)])
    out = []
    for i in range(count):
        snr_db = SNRS_DB[i % len(SNRS_DB)]
        delay = float(rng.uniform(-3.0, 3.0) * sps)
        # every other window sits on a DC offset of the signal's own size, a different one each: whatever a kernel sums
        # from outside its own window then moves its mean visibly.  (No larger: the reference sums the mean in fp32, one
        # sample after the other, and an offset of 25 on 936 samples costs its SNR 7e-5 relative -- the oracle's own
        # rounding would then fill a third of the contract's 2e-4.)
        dc = complex(rng.standard_normal(), rng.standard_normal()) * float(rng.choice([0.5, 1.5])) * (i & 1)
        sign = 1.0 if rng.random() < 0.5 else -1.0
        if cls == "loop":
            cfo = sign * float(rng.uniform(100.0, 2000.0))            # the +-2 kHz of the generators
        elif cls == "edge":
            cfo = float(rng.uniform(-100.0, 100.0))
        else:
            cfo = float(rng.uniform(-2000.0, 2000.0))
        x = make_burst(rng, which, sps, snr_db, cfo, delay, dc)
        if cls == "none":
            fs = None
        elif cls == "zero":
            fs = F32(0.0)
        elif cls == "small":
            fs = F32(sign * 0.02)
        elif cls == "loop":
            # what the receive loop passes (gmr1_rx.c:682): minus the fine estimate of this very burst
            fs = F32(-fine(x, sps, None, which)["freq_error"])
        else:
            # near the end of what fine can return: the burst comes out of the rotation 0.95 pi rad / symbol off
            fs = F32(sign * 0.95 * np.pi * rng.uniform(0.995, 1.005))
        out.append(dict(x=x, fs=fs, snr_db=snr_db, cfo_hz=cfo))
    return out


def flat_layout(cases, sps, fill=complex(90.0, -70.0), tail=1024):
    """All windows in one flat array at odd offsets that are no multiples of sps, the gaps and a tail filled with a
    value far above any signal -> (iq complex64, offset uint64)"""
    pos, offs = 1, []
    for c in cases:
        while pos % 2 == 0 or (sps > 1 and pos % sps == 0):
            pos += 1
        offs.append(pos)
        pos += c["x"].size + 1
    iq = np.full(pos + tail, fill, np.complex64)
    for c, o in zip(cases, offs):
        iq[o:o + c["x"].size] = c["x"]
    return iq, np.array(offs, np.uint64)


def pool_map(fn, items):
    """fn over items on a few threads (the oracle's calls release the interpreter lock and share no state)"""
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(fn, items))


def oracle_all(orc, cases, sps, which):
    """[(fine rv, toa, freq_error, snr rv, snr)] from the oracle"""
    def one(c):
        fs = 0.0 if c["fs"] is None else float(c["fs"])
        return orc.fcch_fine(c["x"], sps, fs, which=which) + orc.fcch_snr(c["x"], sps, fs, which=which)
    return pool_map(one, cases)


def f64_all(cases, sps, which):
    return [(fine(c["x"], sps, c["fs"], which), snr(c["x"], sps, c["fs"], which)[1]) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# HALF_DELTA: how close to a half-integer toa_samples has to be for the oracle's fp32 chain to round the other way
# ---------------------------------------------------------------------------------------------------------------------
def measure_half_delta(orc, seed=20261, n_random=20000, n_steered=400):
    """Largest distance of the restatement's toa_samples from a half-integer at which the oracle returns the other
    integer, over (1) n_random bursts drawn across the grid (all types, sps, shift classes; FCCH3 thinned to a fifth:
    the oracle's DFT is quadratic), decidable by margin, and (2) n_steered bursts whose delay is bisected until
    toa_samples sits on a half-integer and then stepped across it in a ladder of 1e-7 ... 4e-3 samples, so that the
    band where the two disagree is actually sampled.  Returns (figure, disagreements, bursts compared)."""
    rng = np.random.default_rng(seed)
    types = list(TYPES)
    todo = []
    while len(todo) < n_random:
        which = types[0] if rng.random() < 0.8 else types[int(rng.integers(1, 3))]
        sps = int(rng.choice(SPS_GRID))
        cls = SHIFT_CLASSES[int(rng.integers(0, len(SHIFT_CLASSES)))]
        for c in cell_cases(which, sps, cls, count=25, seed=int(rng.integers(1 << 30))):
            todo.append((which, sps, c))
    for _ in range(n_steered):
        which = types[0] if rng.random() < 0.8 else types[int(rng.integers(1, 3))]
        sps = int(rng.choice(SPS_GRID))
        snr_db = SNRS_DB[int(rng.integers(0, len(SNRS_DB)))]
        cfo = float(rng.uniform(-2000.0, 2000.0))
        s = int(rng.integers(1 << 30))

        def at(delay):
            x = make_burst(np.random.default_rng(s), which, sps, snr_db, cfo, delay, 0.0)
            return x, fine(x, sps, None, which)["toa_samples"]
        target = np.floor(rng.uniform(-2.0, 2.0) * sps) + 0.5
        lo, hi = target - 2.0, target + 2.0                           # toa_samples follows the delay, slope about one
        if not (at(lo)[1] < target < at(hi)[1]):
            continue
        for _ in range(40):
            m = 0.5 * (lo + hi)
            lo, hi = (m, hi) if at(m)[1] < target else (lo, m)
        if abs(at(lo)[1] - target) > 1e-6:
            continue                                                  # a jump of toa_samples (the best window moved), no crossing
        for step in (1e-7, 1e-6, 1e-5, 3e-5, 1e-4, 2e-4, 3e-4, 4.5e-4, 6e-4, 8e-4, 1e-3, 1.5e-3, 2e-3, 4e-3):
            for sg in (-1.0, 1.0):
                todo.append((which, sps, dict(x=at(lo + sg * step)[0], fs=None)))

    def one(t):
        which, sps, c = t
        f = fine(c["x"], sps, c["fs"], which)
        if f["toa"] is None or f["margin"] < MARGIN_MIN:
            return None
        o = orc.fcch_fine(c["x"], sps, 0.0 if c["fs"] is None else float(c["fs"]), which=which)
        ts = f["toa_samples"]
        return (o[1] != f["toa"], abs(abs(ts - np.floor(ts)) - 0.5), abs(o[1] - f["toa"]))
    res = [r for r in pool_map(one, todo) if r is not None]
    assert all(r[2] <= 1 for r in res), "the oracle and the restatement differ by more than one rounding"
    bad = [r[1] for r in res if r[0]]
    return (max(bad) if bad else 0.0), len(bad), len(res)


if __name__ == "__main__":
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_lib
    oracle_lib.build()
    oracle_lib.lib()
    if "--sweep" in sys.argv:
        n = int(sys.argv[sys.argv.index("--sweep") + 1]) if len(sys.argv) > sys.argv.index("--sweep") + 1 else 20000
        t0 = time.time()
        print("half delta measured %.3e samples: %d disagreements in %d bursts (%.0f s)"
              % (measure_half_delta(oracle_lib, n_random=n) + (time.time() - t0,)))
