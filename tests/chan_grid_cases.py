"""What tests/test_gpu_chan_grid.py (GPU) and tests/test_chan_grid_host.py (no GPU) share: the grid's cells, its signals, a
Python restatement of the resampler's launch rule (osmo-gmr_amd/csrc/chan_select.h), a float32 restatement of the
channelizer chain, and the mutations of the float64 reference that show what the rounding-scale bound can see.

Two bounds per compared sample:
  the contract        |product - oracle| < 2e-4 max(1, rms(oracle))
  the rounding scale  |product - oracle| <= 8 max|f32 restatement - oracle|   per cell and channel
The product and the restatement are two float32 evaluations of the same sums in different orders, so their errors are draws
from the same envelope; the restatement does not round the DFT's six stages and the kernels fuse their multiply-adds: three
doublings cover that.  The float64 oracle (oracle/orc_chan.py) stays the reference of both."""
import functools
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import orc_chan  # noqa: E402

FS = 2.0e6
CHANS = [5, 40, 31, 0, 63, 32]
N_GRID = 661237                    # 33 periods of 20 000 wideband samples and a ragged 34th; T = 20 663 is odd
CONTRACT = 2e-4
ROUNDING_FACTOR = 8.0
MUTATION_FACTOR = 10.0
NFILT = 32
PERIODS, PERIODS_STREAM = 32, 4    # kRsPeriods, kRsPeriodsStream


# ---------------------------------------------------------------------------------------------------------- the rule
def resamp_form(step, tpf, T, n_out, ext=False, stream=False, o0=0, planar=False, one_only=False, shared_ring=False,
                wg1=False):
    """chan_select.h's resamp_choice, restated with exact fractions: step = num / den (in 1 / 32 input samples per output).
    The outputs of a wave's lanes 0 .. 63 (.. 127 with two per lane) start floor(63 r) (floor(127 r)) inputs apart at
    r = step / 32 inputs per output; each reads `taps` samples back, and two more cover the rounding of both ends."""
    r = Fraction(step) / NFILT                                   # input samples per output
    P, Q = r.denominator, r.numerator                            # the phase repeats every P outputs = Q inputs
    taps = 96 if tpf == 96 else 30
    span = math.floor(63 * r) + taps + 2
    span_r = math.floor(127 * r) + taps + 2
    c = dict(P=P, Q=Q, span=span, span_r=span_r, taps=taps, ext=ext)
    if n_out <= (o0 if stream else 0):
        return dict(c, form="none")
    if (tpf not in (30, 96) or span > (512 if taps == 96 else 256) or (taps == 96 and ext)
            or (stream and (o0 < 0 or planar))):
        return dict(c, form="refused")
    per = PERIODS_STREAM if stream else PERIODS
    periods = -(-n_out // P) - (o0 // P if stream else 0)
    c["gz"] = -(-periods // per)
    two = (not stream and taps == 30 and not ext and not one_only and r < 1 and span_r <= 128 and T >= 2)
    if not two:
        win = 512 if taps == 96 else (128 if span <= 128 else 256)
        return dict(c, form="k_resamp<%d,%d%s>" % (taps, win, ",EXT" if ext else ""), win=win, wg=1, gx=-(-P // 64),
                    per_lane=1)
    gx2 = -(-P // 128)
    nch = -(-(math.floor(1023 * r) + taps + 2) // 128)
    if shared_ring and nch < 8 and gx2 >= 8:
        return dict(c, form="k_resamp2w", win=128, wg=8, gx=-(-gx2 // 8), per_lane=2, nch=nch)
    wg = 1 if wg1 else 8 if gx2 % 8 == 0 else 4 if gx2 % 4 == 0 else 2 if gx2 % 2 == 0 else 1
    return dict(c, form="k_resamp2<WG=%d>" % wg, win=128, wg=wg, gx=gx2 // wg, per_lane=2)


# sps: (P, Q, the span the form is launched with, form) on the filterbank path (2 x 31 250 Hz -> 23 400 sps Hz), by hand:
# r = 62 500 / (23 400 sps) inputs per output = 625 / (234 sps) reduced, span = floor(63 r) + 32 (one output per lane),
# floor(127 r) + 32 (two), groups of 128 outputs per period -> the largest of 8, 4, 2 that divides their count
FILTERBANK = {
    1: (234, 625, 200, "k_resamp<30,256>"), 2: (468, 625, 116, "k_resamp<30,128>"), 3: (702, 625, 88, "k_resamp<30,128>"),
    4: (936, 625, 116, "k_resamp2<WG=8>"), 5: (234, 125, 99, "k_resamp2<WG=2>"), 6: (1404, 625, 88, "k_resamp2<WG=1>"),
    7: (1638, 625, 80, "k_resamp2<WG=1>"), 8: (1872, 625, 74, "k_resamp2<WG=1>"), 9: (2106, 625, 69, "k_resamp2<WG=1>"),
    10: (468, 125, 65, "k_resamp2<WG=4>"), 11: (2574, 625, 62, "k_resamp2<WG=1>"), 12: (2808, 625, 60, "k_resamp2<WG=2>"),
    13: (3042, 625, 58, "k_resamp2<WG=8>"), 14: (3276, 625, 56, "k_resamp2<WG=2>"), 15: (702, 125, 54, "k_resamp2<WG=2>"),
    16: (3744, 625, 53, "k_resamp2<WG=2>"),
}

def plan_runs(step, tpf):
    """chan_select.h's resamp_plan_runs"""
    if tpf not in (30, 96):
        return False
    span = (63 * step.numerator) // (step.denominator * NFILT) + tpf + 2
    return span <= (512 if tpf == 96 else 256)


def fb_step(sps):
    """the filterbank path: 2 x 31 250 Hz channel streams -> 23 400 sps Hz"""
    return Fraction(NFILT * 62500, orc_chan.SYM_RATE * sps)


def pre_step(fs):
    pl = orc_chan.Plan(fs)
    return Fraction(NFILT) / pl.pre_rate


def resamp_count(step, j0, T):
    v = (T * NFILT - j0) * step.denominator
    return v // step.numerator if v > 0 else 0


RRC_J0 = 22                        # (941 // 2) % 32: the filterbank path's first filter


def direct_numbers(fs, sps):
    """The direct mode's plan without its filters (DirectOutputParameters :611-680 as orc_chan.DirectPlan restates it):
    (d1, d2, step, taps per phase, taps of the two FIRs), or None where the plan is refused for another reason than its
    span: an exact multiple of the output rate, no decimation, a resampling rate of 1, a FIR past the 256 taps the kernel
    stages, a bank past 96 taps per phase."""
    sym = orc_chan.SYM_RATE
    if fs % (sym * sps) == 0:
        return None
    lo, hi = int(math.ceil(fs / (3 * sym))), int(math.floor(fs / (2 * sym)))
    cands = [orc_chan.DirectPlan._factor(i) for i in range(lo, hi + 1)]
    if not cands:
        return None
    best = (sorted(cands, key=lambda f: -orc_chan.DirectPlan._score(f))[0] + [1])[0:2]
    resamp = (1.0 * sym * sps * best[0] * best[1]) / fs
    if best[1] <= 4:
        resamp /= best[1]
        best[1] = 1
    if resamp == 1.0:
        return None
    d1, d2 = best
    fs2 = fs / (d1 * d2)
    nt = int(11.0 * 32 * fs2 / sym) | 1
    tpf = -(-nt // NFILT)

    def lp_taps(tw):
        n = int(53.0 / (22.0 * tw))
        return n | 1

    nt1, nt2 = lp_taps(0.3 / d1), lp_taps(0.10 / d2) if d2 != 1 else 0
    if nt1 > 256 or nt2 > 256 or tpf > 96:
        return None
    return d1, d2, Fraction(NFILT * int(fs), d1 * d2 * sym * sps), tpf, nt


class Direct:
    """numbers of a direct-mode plan: the decimations (orc_chan.DirectPlan), the resampler's step, bank and whether the
    kernels run it"""

    def __init__(self, fs, sps):
        self.fs, self.sps = fs, sps
        self.pl = orc_chan.DirectPlan(fs, sps)
        self.d1, self.d2 = self.pl.decim1, self.pl.decim2
        self.step = Fraction(NFILT * int(fs), self.d1 * self.d2 * orc_chan.SYM_RATE * sps)
        nt = self.pl.taps_resamp.size
        self.tpf = -(-nt // NFILT)
        self.bank = 30 if self.tpf <= 30 else 96
        self.j0 = (nt // 2) % NFILT
        assert direct_numbers(fs, sps) == (self.d1, self.d2, self.step, self.tpf, nt)
        self.runs = self.tpf <= 96 and plan_runs(self.step, self.bank)

    def n_out(self, n_in):
        return resamp_count(self.step, self.j0, n_in // self.d1 // self.d2)

    def form(self, n_in):
        return resamp_form(self.step, self.bank, n_in // self.d1 // self.d2, self.n_out(n_in))


# ---------------------------------------------------------------------------------------------------------- signals
def capture(n, fs=FS, seed=2, n_chans=64):
    """noise of deviation 0.3 plus the three tones of test_channelizer_matches_oracle (on the same raster positions counted
    from either end where the plan has another channel count)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 2)) * 0.3).astype(np.float32).view(np.complex64).reshape(-1)
    s = np.arange(n, dtype=np.float64)
    for k, f, a in tones(n_chans):
        kk = k if k < n_chans // 2 else k - n_chans
        x += (a * np.exp(2j * np.pi * np.mod(((kk * 31250.0 + f) / fs) * s, 1.0))).astype(np.complex64)
    return x


def tones(n_chans=64):
    return ((5, 1000.0, 1.0), (n_chans - 24, -4000.0, 0.5), (n_chans // 2 - 1, 9000.0, 2.0))


def chans_of(n_chans):
    return CHANS if n_chans == 64 else [5, n_chans - 24, n_chans // 2 - 1, 0, n_chans - 1, n_chans // 2]


DDC_FREQS = [3 * 31250.0, -7 * 31250.0 + 400.0, 0.0]


def ddc_capture(n, fs, seed):
    """the existing direct-mode test's three carriers, 900 Hz off each"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 2)) * 0.3).astype(np.float32).view(np.complex64).reshape(-1)
    s = np.arange(n, dtype=np.float64)
    for f, a in zip(DDC_FREQS, (1.0, 0.6, 1.5)):
        x += (a * np.exp(2j * np.pi * np.mod(((f + 900.0) / fs) * s, 1.0))).astype(np.complex64)
    return x


# ---------------------------------------------------------------------------------------------------------- the chain
def _banks(taps, dtype):
    """bank[j, k] = taps[j + 32 k] and the first-difference bank (the last difference 0), in `dtype`"""
    nt = taps.size
    tpf = -(-nt // NFILT)
    tp = np.zeros(tpf * NFILT, dtype)
    tp[:nt] = taps
    dt = np.zeros_like(tp)
    dt[:nt - 1] = tp[1:nt] - tp[:nt - 1]
    return tp.reshape(tpf, NFILT).T, dt.reshape(tpf, NFILT).T, tpf


def resample(x, step, taps, n_out, f32=False, mut=None):
    """orc_chan.arb_resampler in its own summation order, float64 (bit for bit the oracle's, which the host test checks) or
    float32: taps b + frac d formed first, products and sums in float32.  mut: one of MUTATIONS, applied to the float64 form."""
    taps = np.asarray(taps, np.float32).copy()
    nt = taps.size
    j0 = (nt // 2) % NFILT
    num, den = step.numerator, step.denominator
    n = np.arange(n_out, dtype=np.int64)
    N = j0 * den + n * num
    fl = N // den
    rem = N % den
    if mut == "frac_next":
        rem = (j0 * den + (n + 1) * num) % den
    j = fl % NFILT
    if mut in ("first_tap", "last_tap"):
        # the first / last tap of the prototype that the plan reads: tap 0 / the last one wherever the phase walks all 32
        # filters; a short period (27 outputs at 1.3 Msps, sps 3) never uses some, and a tap nobody reads is no mutation
        used = np.unique(j)
        if mut == "first_tap":
            taps[used.min()] = 0.0
        else:
            last = max(int(u) + NFILT * ((nt - 1 - int(u)) // NFILT) for u in used)
            taps[min(last + 1, nt - 1)] = 0.0                        # (tap i + 1 is read through the difference d[i])
    if mut == "j_off":
        j = np.where(n % 64 == 63, (j + 1) % NFILT, j)
    i_in = fl // NFILT
    if f32:
        bank, dbank, tpf = _banks(taps, np.float32)
        frac = rem.astype(np.float32) / np.float32(den)
        e = bank[j] + frac[:, None] * dbank[j]                       # float32 throughout
        xp = np.concatenate([np.zeros(tpf, np.complex64), np.asarray(x, np.complex64), np.zeros(tpf + 2, np.complex64)])
        acc = np.zeros(n_out, np.complex64)
        for k in range(tpf):
            acc += e[:, k] * xp[i_in - k + tpf]
        return acc
    bank, dbank, tpf = _banks(taps.astype(np.float64), np.float64)
    frac = rem.astype(np.float64) / den
    if mut == "no_deriv":
        frac = np.zeros_like(frac)
    xp = np.concatenate([np.zeros(tpf, np.complex128), np.asarray(x, np.complex128), np.zeros(tpf + 2, np.complex128)])
    o0 = np.zeros(n_out, np.complex128)
    o1 = np.zeros(n_out, np.complex128)
    for k in range(tpf):
        s = xp[i_in - k + tpf]
        o0 += bank[j, k] * s
        o1 += dbank[j, k] * s
    return (o0 + o1 * frac).astype(np.complex64)


MUTATIONS = ("last_tap", "first_tap", "no_deriv", "frac_next", "j_off")


def pfb_f32(x, taps, n_chans):
    """orc_chan.pfb_channelizer_2x with the branch FIR's products and sums in float32, in the oracle's order (blocks from the
    oldest); the DFT in double, its output rounded to float32"""
    M, D = n_chans, n_chans // 2
    x = np.asarray(x, np.complex64)
    L = taps.size
    P = -(-L // M) + 1
    T = x.size // D
    h = np.zeros(P * M + M, np.float32)
    h[:L] = taps
    xp = np.concatenate([np.zeros(P * M, np.complex64), x, np.zeros(M, np.complex64)])
    out = np.empty((M, T), np.complex64)
    r = np.arange(M)
    for par in range(2):
        ts = np.arange(par, T, 2)
        if ts.size == 0:
            continue
        v = np.zeros((ts.size, M), np.complex64)
        for q in range(-P, 1):
            blk = (ts * D) // M + q
            s = blk[:, None] * M + r[None, :]
            ti = (ts * D)[:, None] - s
            ok = (ti >= 0) & (ti < L)
            v += np.where(ok, xp[s + P * M] * h[np.clip(ti, 0, L - 1)], np.complex64(0))
        out[:, ts] = np.fft.fft(v.astype(np.complex128), axis=1).T.astype(np.complex64)
    return out


def fir_f32(x, taps, decim):
    """orc_chan.fir_decimate with complex or real float32 taps, products and sums in float32, taps from k = 0"""
    x = np.asarray(x, np.complex64)
    taps = np.asarray(taps)
    n_out = x.size // decim
    xp = np.concatenate([np.zeros(taps.size, np.complex64), x])
    m = np.arange(n_out, dtype=np.int64) * decim + taps.size
    acc = np.zeros(n_out, np.complex64)
    for k in range(taps.size):
        acc += taps[k].astype(np.complex64 if np.iscomplexobj(taps) else np.float32) * xp[m - k]
    return acc


def ddc_stages(x, d, freq_hz, f32=False):
    """the direct mode's stream in front of its resampler (orc_chan.direct_ddc's two FIRs).  float32: as the product forms
    it -- the low-pass turned up to the carrier in double and rounded (the taps the library uploads), the output turned back
    with an angle reduced in double"""
    pl = d.pl
    if not f32:
        xx = np.asarray(x, np.complex128)
        z = xx * np.exp(-2j * np.pi * (freq_hz / pl.samp_rate) * np.arange(xx.size))
        y = orc_chan.fir_decimate(z, pl.taps1, pl.decim1)
        if pl.decim2 > 1:
            y = orc_chan.fir_decimate(y, pl.taps2, pl.decim2)
        return y
    fn = freq_hz / pl.samp_rate
    k = np.arange(pl.taps1.size)
    ph = 2.0 * np.pi * np.mod(fn * k, 1.0)
    t1 = (pl.taps1.astype(np.float64) * np.exp(1j * ph)).astype(np.complex64)
    y = fir_f32(x, t1, pl.decim1)
    m = np.arange(y.size, dtype=np.float64)
    rot = np.exp(-2j * np.pi * np.mod(m * (fn * pl.decim1), 1.0).astype(np.float32).astype(np.float64)).astype(np.complex64)
    y = y * rot
    if pl.decim2 > 1:
        y = fir_f32(y, pl.taps2, pl.decim2)
    return y


def bounds(ref, f32):
    """(contract, rounding scale) of one channel: what |product - ref| is held to"""
    ref = np.asarray(ref)
    rms = float(np.sqrt(np.mean(np.abs(ref) ** 2))) if ref.size else 0.0
    e32 = float(np.max(np.abs(np.asarray(f32) - ref))) if ref.size else 0.0
    return CONTRACT * max(1.0, rms), ROUNDING_FACTOR * e32


# ---------------------------------------------------------------------------------------------------------- short captures
SHORT_T = (0, 1, 2, 3, 29, 30, 31, 63, 64, 65, 127, 128, 129, 160)
SHORT_SPS = (1, 4, 16)


def short_lengths():
    """n_in of the short captures at 2.0 Msps: T = n_in // 32"""
    return [0, 31] + [32 * T + 17 for T in SHORT_T if T]


SHORT_ANY_T = (0, 1, 2, 129)           # 1.25 Msps (40 channels: T = n_in // 20)
SHORT_DDC_N = (0, 41, 42, 83, 84, 42 * 31 + 5)

# ---------------------------------------------------------------------------------------------------------- direct mode
DDC_RATES = (2.0e6, 1.25e6, 1.0e6, 2.5e6)
DDC_SPS = (1, 2, 3, 5, 8, 16)
# what tests/c/chan_select_host.cpp's search over the multiples of 10 kHz from 0.5 to 8 Msps x sps 1 .. 16 prints (the host
# test holds this table against the program's output and against Direct above):
#   the accepted plan with the largest span_r <= 128, the accepted plan with the largest span <= 512 on the 96-tap bank,
#   the rejected plan nearest above the 512-sample window (none is rejected above the 256-sample one)
DDC_SEARCH = dict(two_widest=(1.3e6, 3), long_widest=(0.92e6, 1), long_refused=(0.62e6, 1))


def ddc_length(d):
    """wideband samples of a direct-mode cell: at least one whole resampler period and a ragged second; 33 periods and a tail
    where that stays under 700 000 samples"""
    f = resamp_form(d.step, d.bank, 1 << 30, 1 << 30)
    per_in = f["Q"] * d.d1 * d.d2                  # wideband samples per resampler period
    n33 = 33 * per_in + per_in // 3 + 5
    if n33 < 700000:
        return n33
    return per_in + per_in // 2 + 5


# ---------------------------------------------------------------------------------------------------------- cells
@functools.lru_cache(maxsize=None)
def fb_front(fs=FS, n=N_GRID, seed=2):
    """(capture, plan, {channel: 2x oversampled stream} in float64, the same in float32) of a filterbank front end -- computed
    once per process: it does not depend on sps.  Off the grid the pre-resampler comes first (both forms)."""
    pl = orc_chan.Plan(fs)
    x = capture(n, fs, seed, pl.n_chans)
    x64, x32 = x, x
    if pl.pre_rate is not None:
        st = Fraction(NFILT) / pl.pre_rate
        n_pre = resamp_count(st, (pl.taps_pre.size // 2) % NFILT, n)
        x64 = resample(x, st, pl.taps_pre, n_pre)
        x32 = resample(x, st, pl.taps_pre, n_pre, f32=True)
    y64 = orc_chan.pfb_channelizer_2x(x64, pl.taps, pl.n_chans)
    y32 = pfb_f32(x32, pl.taps, pl.n_chans)
    ch = chans_of(pl.n_chans)
    for a in (x, y64, y32):
        a.setflags(write=False)
    return x, pl, {k: y64[k] for k in ch}, {k: y32[k] for k in ch}


def fb_cell(sps, fs=FS, n=N_GRID, seed=2):
    """-> (n_out, {channel: oracle stream}, {channel: float32 restatement}) of a filterbank cell"""
    x, pl, y64, y32 = fb_front(fs, n, seed)
    st = fb_step(sps)
    T = next(iter(y64.values())).size
    n_out = resamp_count(st, RRC_J0, T)
    ref = {k: resample(v, st, pl.taps_resamp, n_out) for k, v in y64.items()}
    r32 = {k: resample(v, st, pl.taps_resamp, n_out, f32=True) for k, v in y32.items()}
    return n_out, ref, r32


@functools.lru_cache(maxsize=None)
def ddc_front(fs, n, seed=None):
    """(capture, [per carrier: the stream in front of the resampler, float64], [the same in float32]) of a direct-mode rate:
    the decimations do not depend on sps.  n: the longest capture the rate's cells need; shorter cells take its head (both
    FIRs are causal)."""
    d = Direct(fs, 2)
    x = ddc_capture(n, fs, int(fs) % 97 if seed is None else seed)
    y64 = [ddc_stages(x, d, f) for f in DDC_FREQS]
    y32 = [ddc_stages(x, d, f, f32=True) for f in DDC_FREQS]
    x.setflags(write=False)
    return x, y64, y32


def ddc_cells():
    """(rate, sps) of the direct-mode grid: DDC_RATES x DDC_SPS and what the search found; the refused among them included"""
    cells = [(fs, sps) for fs in DDC_RATES for sps in DDC_SPS]
    return cells + [v for v in DDC_SEARCH.values() if v not in cells]


def ddc_rate_length(fs):
    return max(ddc_length(Direct(f, s)) for f, s in ddc_cells() if f == fs and Direct(f, s).runs)


def ddc_cell(fs, sps):
    """-> (capture, n_out, [oracle stream per carrier], [float32 restatement per carrier])"""
    d = Direct(fs, sps)
    n = ddc_length(d)
    x, y64, y32 = ddc_front(fs, ddc_rate_length(fs))
    T = n // d.d1 // d.d2
    n_out = d.n_out(n)
    ref = [resample(y[:T], d.step, d.pl.taps_resamp, n_out) for y in y64]
    r32 = [resample(y[:T], d.step, d.pl.taps_resamp, n_out, f32=True) for y in y32]
    return x[:n], n_out, ref, r32


# ---------------------------------------------------------------------------------------------------------- coverage
# what the cells together must reach, so that a change to the rule cannot leave a form silently uncovered
REQUIRED_FORMS = {"k_resamp<30,256>", "k_resamp<30,128>", "k_resamp2<WG=1>", "k_resamp2<WG=2>", "k_resamp2<WG=4>",
                  "k_resamp2<WG=8>", "k_resamp2<WG=8> x3", "k_resamp<96,512>", "k_resamp<30,128,EXT>", "k_resamp<30,256,EXT>"}
OTHER_FRONT_ENDS = ((1.25e6, 412500 + 4177), (2.048e6, 675840 + 6151))     # 33 periods of the resampler and a tail
OTHER_SPS = (1, 3, 13)


def grid_forms():
    """the forms of the GPU grid's oracle cells, from the rule alone ("... x3": more than one work-group per period)"""
    forms = set()

    def add(f):
        forms.add(f["form"])
        if f["form"].startswith("k_resamp2") and f["gx"] > 1:
            forms.add("%s x%d" % (f["form"], f["gx"]))

    T = N_GRID // 32
    for sps in range(1, 17):
        st = fb_step(sps)
        n_out = resamp_count(st, RRC_J0, T)
        add(resamp_form(st, 30, T, n_out))
        add(resamp_form(st, 30, T, n_out, ext=True, planar=True))
    for fs, sps in ddc_cells():
        d = Direct(fs, sps)
        if d.runs:
            add(d.form(ddc_length(d)))
    return forms
