"""k_detect, k_mod_order and k_dkab against the oracle away from the one point (4 samples per symbol, no freq_shift) where
tests/test_gpu_rx.py and tests/test_gpu_tch.py run them.

The receive loop reaches all three at every sps and with a freq_shift (rx_tch3 hands gmr1_pi4cxpsk_detect and
gmr1_dkab_demod -freq_err).  launch_detect (rx_small_kernels.h) picks k_detect<samples per lane, sps> by in_len and sps; the
cases below, NT3 bursts (117 symbols) in windows of 117 * sps + win samples, reach

    sps  win   in_len  k_detect   k_mod_order          sps  win   in_len  k_detect   k_mod_order
     1     6     123   <16, 0>    <16>                   8   120    1056   <32, 0>    <32>
     2     6     240   <16, 0>    <16>                  16    20    1892   <32, 0>    <32>
     3     7     358   <16, 0>    <16>                  16   200    2072   <64, 0>    <64>
     5    10     595   <16, 0>    <16>                   2  1900    2134   <64, 0>    <64>
     8    12     948   <16, 0>    <16>

(<16, 4> and <32, 4> are what the sps-4 tests of tests/test_gpu_rx.py reach.)  Contracts, as there: detect -- rv, bt_id and
sync_id identical to the oracle's with the same freq_shift, toa within 16 / 1024 of a sample; mod_order -- identical
decisions; DKAB -- rv identical, toa within 2e-3, soft bits within 1 LSB."""
import numpy as np
import pytest

from test_gpu_tch import _dkab_windows

pytestmark = pytest.mark.gpu

SYM_RATE = 23400
NT3 = ["nt3_facch", "nt3_speech"]
# (sps, win): see the table above
DETECT_CASES = [(1, 6), (2, 6), (3, 7), (5, 10), (8, 12), (8, 120), (16, 20), (16, 200), (2, 1900)]


def _nt3_windows(pkg, sps, win, n, seed, esn0_db):
    """n windows holding an NT3 speech or FACCH3 burst (either sync sequence of the FACCH3 format) half a window in, a
    sample or so of jitter with a fraction, a carrier offset of some hundred Hz -> (iq[n, in_len], truth, cfo rad / sample)"""
    rng = np.random.default_rng(seed)
    fmts = [pkg.api.burst_format(b) for b in NT3]
    in_len = 117 * sps + win
    iq = np.zeros((n, in_len), np.complex64)
    truth = np.zeros(n, int)
    cfo = np.zeros(n)
    for i in range(n):
        truth[i] = int(rng.integers(0, 2))
        fmt = fmts[truth[i]]
        bits = rng.integers(0, 2, (1, fmt.ebits), dtype=np.uint8)
        sym = pkg.synth.map_symbols(fmt, bits, sync_id=int(rng.integers(0, len(fmt.sync))))
        bb = pkg.synth.synth_windows(fmt, sym, sps, win, rng, toa_jitter=min(1, win // 4), frac=True, cfo_hz_std=300.0,
                                     esn0_db=esn0_db)
        iq[i] = bb.iq[0, :in_len]
        cfo[i] = bb.cfo[0]
    return iq, truth, cfo


def _shifts(sps, cfo, seed):
    """per burst: the shift that takes the synthesised carrier offset out (what rx_tch3 passes), and an unrelated one"""
    rng = np.random.default_rng(seed)
    return {"matching": (-cfo * sps).astype(np.float32), "unrelated": rng.normal(0.0, 0.08, cfo.size).astype(np.float32)}


@pytest.mark.parametrize("sps,win", DETECT_CASES)
def test_detect_grid(gpu_api, orc, pkg, sps, win):
    n = 40
    iq, truth, cfo = _nt3_windows(pkg, sps, win, n, seed=1000 + 16 * win + sps, esn0_db=15.0)
    in_len = iq.shape[1]
    offset = (np.arange(n) * in_len).astype(np.uint64)
    for kind, fs in _shifts(sps, cfo, seed=sps).items():
        for e_toa in (win / 2.0, None):
            got = gpu_api.detect_batch(NT3, iq, offset, in_len, sps=sps, freq_shift=fs, e_toa=e_toa)
            for i in range(n):
                o = orc.detect(NT3, -1.0 if e_toa is None else e_toa, iq[i], sps, float(fs[i]))
                tag = (sps, win, kind, e_toa, i)
                assert got["rv"][i] == o["rv"] == 0, tag
                assert got["bt_id"][i] == o["bt_id"], (tag, got["bt_id"][i], o)
                assert got["sync_id"][i] == o["sync_id"], (tag, got["sync_id"][i], o)
                assert abs(got["toa"][i] - o["toa"]) < 16 / 1024, (tag, got["toa"][i], o)
            if kind == "matching" and e_toa is not None and win <= 20 and sps >= 2:
                # what tests/test_gpu_rx.py demands of the estimator at sps 4: with the expected toa, a window a few symbols
                # wide and more than one sample per symbol (the oracle itself is right 85 % of the time at sps 1, and 60 %
                # in the 1900-sample window without an expected toa: the correlation has that many noise lags to choose from)
                assert (got["bt_id"] == truth).mean() > 0.9, (sps, win, e_toa)
        # the reference's own call, the shift as its C float
        for i in range(0, n, 9):
            d = gpu_api.pi4cxpsk_detect(NT3, win / 2.0, iq[i], sps, float(fs[i]))
            o = orc.detect(NT3, win / 2.0, iq[i], sps, float(fs[i]))
            assert (d["rv"], d["bt_id"], d["sync_id"]) == (0, o["bt_id"], o["sync_id"]), (sps, win, kind, i, d, o)
            assert abs(d["toa"] - o["toa"]) < 16 / 1024


@pytest.mark.parametrize("sps,win", [(3, 7), (16, 200)])
def test_detect_long_list_at_generic_sps(gpu_api, orc, pkg, sps, win):
    """more than four candidates: a second launch of a generic-sps instantiation (<16, 0> and <64, 0>) takes over the best
    so far from the first (the carry), with a per-burst freq_shift; the winner is the oracle's on the same list"""
    n = 30
    iq, truth, cfo = _nt3_windows(pkg, sps, win, n, seed=77 + sps, esn0_db=15.0)
    in_len = iq.shape[1]
    offset = (np.arange(n) * in_len).astype(np.uint64)
    fs = _shifts(sps, cfo, seed=5)["matching"]
    long_list = ["nt3_speech", "nt3_speech", "nt3_speech", "nt3_speech", "nt3_facch", "nt3_speech", "nt3_facch"]
    for e_toa in (win / 2.0, None):
        got = gpu_api.detect_batch(long_list, iq, offset, in_len, sps=sps, freq_shift=fs, e_toa=e_toa)
        for i in range(n):
            o = orc.detect(long_list, -1.0 if e_toa is None else e_toa, iq[i], sps, float(fs[i]))
            assert (got["rv"][i], got["bt_id"][i], got["sync_id"][i]) == (0, o["bt_id"], o["sync_id"]), (sps, e_toa, i, o)
            assert abs(got["toa"][i] - o["toa"]) < 16 / 1024
            assert got["bt_id"][i] in (0, 4)               # the first copy of either format: a later one never beats it
        assert set(got["bt_id"]) == {0, 4}                 # (a FACCH3 can only win from the second launch, and does)


@pytest.mark.parametrize("sps,win", DETECT_CASES)
def test_mod_order_grid(gpu_api, orc, pkg, sps, win):
    n = 40
    iq, truth, cfo = _nt3_windows(pkg, sps, win, n, seed=2000 + 16 * win + sps, esn0_db=15.0)
    in_len = iq.shape[1]
    offset = (np.arange(n) * in_len).astype(np.uint64)
    shifts = _shifts(sps, cfo, seed=sps + 50)
    shifts["none"] = None
    for kind, fs in shifts.items():
        order = gpu_api.mod_order_batch(iq, offset, in_len, sps=sps, freq_shift=fs)
        for i in range(n):
            want = orc.mod_order(iq[i], sps, 0.0 if fs is None else float(fs[i]))
            assert order[i] == want, (sps, win, kind, i, order[i], want)
        if kind == "matching":
            # the rate tests/test_gpu_rx.py demands of the estimator (there at 8 and 15 dB, here at 15)
            assert (order == np.where(truth == 1, 4, 2)).mean() >= 0.8, (sps, win)
        if fs is not None:
            for i in range(0, n, 9):
                assert gpu_api.pi4cxpsk_mod_order(iq[i], sps, float(fs[i])) == order[i], (sps, win, kind, i)


@pytest.mark.parametrize("sps", [1, 2, 3, 5, 8, 16])
def test_dkab_grid(gpu_api, orc, pkg, sps):
    """gmr1_dkab_demod's offsets sps * (2 + p), sps * (2 + p + 59), d = sps * 5 and the (sps - 1) / 2 timing term at every
    sps the entry point accepts of the grid (all of them); p over its whole range 0 ... 51, the last legal value (the
    second keep-alive burst ends with the window's last symbol) forced onto a tenth of the bursts; shifts mixed, a fifth
    of the windows without a burst."""
    n = 200
    w = 4 if sps == 1 else max(6, 2 * sps)       # (the generator's lead-in is 5 symbols: the search window stays inside it)
    win, ps, bits, present = _dkab_windows(pkg, n, 300 + sps, win=w, p_max=52, sps=sps)
    ps[::10] = 51
    # (p was changed after the synthesis: those windows hold a burst at another p or none, which is as good a case)
    ps2 = ps.copy()
    fresh, _, bits2, present2 = _dkab_windows(pkg, n // 10, 900 + sps, win=w, p_max=52, sps=sps)
    in_len = win.shape[1]
    rng = np.random.default_rng(sps)
    fs = rng.normal(0, 0.02, n).astype(np.float32)
    fs[::7] = 0.0
    offset = np.arange(n, dtype=np.uint64) * np.uint64(in_len)
    rv, eb, toa = gpu_api.dkab_demod_batch(win.reshape(-1), offset, in_len, ps2, sps=sps, freq_shift=fs)
    n_found = 0
    for i in range(n):
        orv, oeb, otoa = orc.dkab_demod(win[i], sps, float(fs[i]), int(ps2[i]))
        assert rv[i] == orv, (sps, i, rv[i], orv)
        assert abs(toa[i] - otoa) < 2e-3, (sps, i, toa[i], otoa)
        if orv == 0:
            n_found += 1
            assert np.max(np.abs(eb[i].astype(int) - oeb.astype(int))) <= 1, (sps, i, eb[i], oeb)
    assert n_found > 0.5 * n
    # bursts really sent at p = 51, found there
    p51 = np.full(fresh.shape[0], 51, np.int32)
    sent = np.zeros_like(fresh)
    synth = pkg.synth
    sigma = np.sqrt(10.0 ** (-20.0 / 10.0) / 2.0)
    for i in range(fresh.shape[0]):
        x = (rng.standard_normal((in_len + 40 * sps, 2)) * sigma).astype(np.float32).view(np.complex64).reshape(-1)
        body = synth.shape_bursts(synth.dkab_symbols(bits2[i:i + 1], 51), sps, float(rng.random()), 5)[0]
        x[:body.size] += body * np.exp(1j * rng.uniform(0, 2 * np.pi))
        sent[i] = x[5 * sps - 2:5 * sps - 2 + in_len]
    off2 = np.arange(sent.shape[0], dtype=np.uint64) * np.uint64(in_len)
    rv, eb, toa = gpu_api.dkab_demod_batch(sent.reshape(-1), off2, in_len, p51, sps=sps)
    for i in range(sent.shape[0]):
        orv, oeb, otoa = orc.dkab_demod(sent[i], sps, 0.0, 51)
        assert rv[i] == orv and abs(toa[i] - otoa) < 2e-3, (sps, i, rv[i], orv, toa[i], otoa)
        if orv == 0:
            assert np.max(np.abs(eb[i].astype(int) - oeb.astype(int))) <= 1, (sps, i, eb[i], oeb)
    assert (rv == 0).mean() > 0.6
    # the reference's own call
    r1, e1, t1 = gpu_api.dkab_demod(win[1], sps, float(fs[1]), int(ps2[1]))
    orv, oeb, otoa = orc.dkab_demod(win[1], sps, float(fs[1]), int(ps2[1]))
    assert r1 == orv and abs(t1 - otoa) < 2e-3 and (r1 or np.max(np.abs(e1.astype(int) - oeb.astype(int))) <= 1)
