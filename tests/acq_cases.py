"""Streams and expected results of the batched FCCH acquisition (gmr1_hip_fcch_acquire_batch*), shared by
tests/test_gpu_fcch_acquire.py.  The expected record of a stream is put together here from the CPU oracle's four FCCH
primitives in the order gmr1_rx runs them (main() -> fcch_single_init -> fcch_multi_process, up to the survivor list)."""
import numpy as np

import workloads

SYM_RATE = 23400
MAX_CHAINS = 16
BURST_LEN = {"fcch": 117, "fcch3_lband": 468, "fcch3_sband": 468}
MARGIN = 0.01          # how far from a threshold every survivor decision of the test streams has to stay


def windows(sps):
    """(samples of the 330 ms window, samples of the 650 ms window)"""
    return (330 * SYM_RATE * sps) // 1000, (650 * SYM_RATE * sps) // 1000


def to_hz(f):
    """gmr1_rx's to_hz in single precision"""
    return (np.float32(SYM_RATE) * np.float32(f)) / (np.float32(2.0) * np.float32(np.pi))


def multi_window(win, sps, which):
    """The 650 ms window as the oracle's rough_multi can be given it.  rough_multi pairs every lag below 7488 + burst with the
    lag one period on, and a period may measure up to 7498.  A 650 ms window has 15210 - burst + 1 lags.  With the 117-symbol
    burst the pairs end at most 8 lags past them, which the oracle holds as zeros (it keeps 64 spare entries) and the product
    takes as zeros.  With the 468-symbol burst they end 711 lags past them: the product still takes zeros, the oracle, like
    gmr1_fcch_rough_multi itself, would read whatever lies behind its array, and its count would depend on that.  So the
    window gets as many zero samples behind it as lags are missing beyond those spare ones: the oracle then pairs with
    lags that it has computed -- zero where the burst lies in the appended part, the window's last samples against the
    head of the burst before that -- and the same window always gives the same peaks."""
    blen = BURST_LEN[which]
    period = (320 * SYM_RATE) // 1000
    lags = win.size // sps - blen + 1
    missing = (period + blen) + (period + 10) - (lags + 64)
    if missing <= 0:
        return win
    return np.concatenate([win, np.zeros(missing * sps, np.complex64)])


def expected(orc, x, sps, start=8000, which="fcch"):
    """-> (record as a dict, margins): what the acquisition has to report for the stream x.  margins: for every candidate
    behind the first, the relative distances of its SNR from 2 and from a sixth of the first one's, and of its frequency
    difference from 500 Hz."""
    f32 = np.float32
    flen = BURST_LEN[which] * sps
    wl1, wl3 = windows(sps)
    n = x.size
    rec = dict(status=0, n_chains=0, align=0, base_align=0, freq_err=f32(0), n_cand=0,
               chain_align=np.zeros(MAX_CHAINS, np.int32), chain_freq_err=np.zeros(MAX_CHAINS, np.float32),
               chain_snr=np.zeros(MAX_CHAINS, np.float32))

    def failed(status):
        rec["status"] = status
        return rec, []

    # the first carrier-wide search: 330 ms from `start`, then the burst found there once more, finely
    if start + wl1 > n:
        return failed(-1)
    rv, toa = orc.fcch_rough(x[start:start + wl1], sps, 0.0, which)
    if rv:
        return failed(rv)
    align = start + toa
    if align + flen > n:
        return failed(-1)
    rv, toa, fe = orc.fcch_fine(x[align:align + flen], sps, 0.0, which)
    assert rv == 0
    align += toa
    fe = f32(fe)
    # every FCCH train in 650 ms from one burst ahead of it
    base = max(0, align - flen)
    if base + wl3 > n:
        return failed(-1)
    cnt, peaks = orc.fcch_rough_multi(multi_window(x[base:base + wl3], sps, which), sps, float(-fe), MAX_CHAINS, which)
    if cnt < 0:
        return failed(cnt)
    # a candidate whose burst does not lie within the stream ends the carrier, as found and as refined
    if any(base + p < 0 or base + p + flen > n for p in peaks):
        return failed(-1)
    fine = []
    for p in peaks:
        rv, ctoa, cfe = orc.fcch_fine(x[base + p:base + p + flen], sps, float(-fe), which)
        assert rv == 0
        fine.append((int(p) + ctoa, f32(cfe)))
    if any(base + q < 0 or base + q + flen > n for q, _ in fine):
        return failed(-1)
    snrs = []
    for q, cfe in fine:
        rv, snr = orc.fcch_snr(x[base + q:base + q + flen], sps, float(-(fe + cfe)), which)
        assert rv == 0
        snrs.append(f32(snr))
    # the first candidate is the yardstick of the others
    keep, margins = [], []
    for i, ((q, cfe), snr) in enumerate(zip(fine, snrs)):
        if i:
            sixth = snrs[0] / f32(6.0)
            hz = to_hz(abs(fine[0][1] - cfe))
            margins.append((abs(snr - 2.0) / 2.0, abs(snr - sixth) / sixth, abs(hz - 500.0) / 500.0))
            if snr < f32(2.0) or snr < sixth or hz > f32(500.0):
                continue
        keep.append(i)
    rec.update(n_chains=len(keep), align=align, base_align=base, freq_err=fe, n_cand=cnt)
    for j, i in enumerate(keep):
        rec["chain_align"][j] = base + fine[i][0]
        rec["chain_freq_err"][j] = fine[i][1]
        rec["chain_snr"][j] = snrs[i]
    return rec, margins


def _shifted(x, delay, hz, sps):
    """x delayed by `delay` samples and moved up by hz"""
    y = np.zeros_like(x)
    y[delay:] = x[:x.size - delay]
    ph = 2.0 * np.pi * hz / (SYM_RATE * sps) * np.arange(x.size)
    return (y * np.exp(1j * ph)).astype(np.complex64)


SPS = 4
N_15 = int(1.5 * SYM_RATE * SPS)          # 140 400 samples

# six carriers that differ in timing, carrier offset and Es/N0
CARRIERS = [dict(seed=501, stn=0, delay=0, cfo_hz=0.0, esn0_db=15.0), dict(seed=502, stn=5, delay=3, cfo_hz=120.0, esn0_db=10.0),
            dict(seed=503, stn=11, delay=7, cfo_hz=-250.0, esn0_db=20.0), dict(seed=504, stn=17, delay=1, cfo_hz=400.0, esn0_db=8.0),
            dict(seed=505, stn=23, delay=5, cfo_hz=-60.0, esn0_db=12.0), dict(seed=506, stn=8, delay=2, cfo_hz=800.0, esn0_db=6.0)]


def carrier(pkg, seed, sps=SPS, seconds=1.5, **kw):
    return workloads.bcch_carrier(pkg, seed, seconds=seconds, sps=sps, **kw)[0]


def plain_streams(pkg):
    """The call with start = NULL: six carriers, noise only, a stream shorter than start + 330 ms, one that holds the 330 ms
    window but not the 650 ms one.  -> list of (name, samples)"""
    out = [("carrier%d" % i, carrier(pkg, **kw)) for i, kw in enumerate(CARRIERS)]
    rng = np.random.default_rng(80)
    out.append(("noise", (rng.standard_normal((N_15, 2), dtype=np.float32).view(np.complex64).reshape(-1)
                          * np.float32(np.sqrt(0.5)))))
    out.append(("short", carrier(pkg, 511)[:30000]))
    out.append(("no650", carrier(pkg, 512)[:50000]))
    return out


def pair_streams(pkg):
    """The call with a start array: sums of two carriers, the second one delayed by a fraction of a frame, moved in
    frequency and weaker -- at 0.2 of the first rough_multi does not report it, at 0.6 it does and the frequency check decides:
    800 Hz away it is dropped, 100 Hz away it is a second chain -- and one carrier searched from another start.  (A candidate
    dropped for its SNR: the sixth carrier and the noise of plain_streams.)  -> list of (name, samples, start)"""
    a = carrier(pkg, 521, stn=2, delay=1, esn0_db=15.0)
    b = carrier(pkg, 522, stn=2, delay=1, esn0_db=15.0)
    frame = 24 * 39 * SPS
    out = []
    for scale in (0.2, 0.6):
        for hz in (800.0, 100.0):
            out.append(("pair_%g_%+dHz" % (scale, hz), (a + np.float32(scale) * _shifted(b, int(0.37 * frame), hz, SPS)), 8000))
    out.append(("late_start", carrier(pkg, **CARRIERS[1]), 23456))
    return out


def fcch3_stream(pkg):
    """One FCCH3 train (468-symbol chirp every 320 ms), built as tests/test_gpu_fcch.py::test_fcch3_long_chirp builds its
    single chirp"""
    rng = np.random.default_rng(9)
    return pkg.synth.synth_fcch_stream(N_15, SPS, rng, snr_db=6.0, cfo_hz=100.0, first=3000, freq=0.32, length=468)[0]


def pack(streams):
    """-> (flat complex64, offset, length) with 64 samples of nothing between two streams"""
    off, pos = [], 0
    for x in streams:
        off.append(pos)
        pos += (x.size + 64 + 15) & ~15
    iq = np.zeros(pos, np.complex64)
    for o, x in zip(off, streams):
        iq[o:o + x.size] = x
    return iq, np.array(off, np.uint64), np.array([x.size for x in streams], np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU tests of the acquisition hold a record to (tests/test_gpu_fcch_acquire.py, tests/test_gpu_fcch_multi.py)
# ---------------------------------------------------------------------------------------------------------------------
INT_FIELDS = ("status", "n_chains", "n_cand", "align", "base_align")


def check_record(name, got, want):
    """one record against the oracle's: integers equal, frequencies within 1e-4, SNR within 2e-4 relative (the bounds of
    tests/test_gpu_fcch.py for the single stages), unused slots exactly 0"""
    for k in INT_FIELDS:
        assert int(got[k]) == int(want[k]), (name, k, int(got[k]), int(want[k]))
    nc = int(want["n_chains"])
    assert list(got["chain_align"]) == list(want["chain_align"]), (name, got["chain_align"], want["chain_align"])
    assert abs(float(got["freq_err"]) - float(want["freq_err"])) < 1e-4, (name, got["freq_err"], want["freq_err"])
    for j in range(nc):
        g, w = float(got["chain_freq_err"][j]), float(want["chain_freq_err"][j])
        assert abs(g - w) < 1e-4, (name, j, g, w)
        g, w = float(got["chain_snr"][j]), float(want["chain_snr"][j])
        assert abs(g - w) <= 2e-4 * max(1.0, abs(w)), (name, j, g, w)
    for k in ("chain_align", "chain_freq_err", "chain_snr"):
        assert not got[k][nc:].view(np.uint32).any(), (name, k, got[k])
    if int(want["status"]):
        assert not bytes(got.tobytes()[4:]).strip(b"\0"), name


def expected_all(orc, cases, sps=None, which="fcch"):
    """[(name, samples, start)] -> the oracle's records; every survivor decision in them is at least MARGIN off its threshold"""
    sps = SPS if sps is None else sps
    want = []
    for name, x, start in cases:
        rec, margins = expected(orc, x, sps, start, which)
        for m in margins:
            assert min(m) >= MARGIN, (name, m)
        want.append(rec)
    return want
