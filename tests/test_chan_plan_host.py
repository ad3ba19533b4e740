"""The channelizer's and the direct mode's plans without a GPU (osmo-gmr_amd/csrc/chan_plan.h through
tests/c/chan_plan_host.cpp): the C++ the library runs -- decimation search, reduced phase steps, counts, the three filter
designs, the polyphase banks, the per-carrier taps, the channel selection and every refusal -- against the restatements the
GPU tests already trust (oracle/orc_chan.py, chan_grid_cases), never by asking the header twice.  Once plain, once under the
address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded).

Taps: both sides compute in double and round once to float32; libm and numpy may differ in the last place of a double, so a
tap may land on the other side of a rounding boundary: one float32 unit in the last place of the tap itself is allowed, no
more (test_the_tap_comparison_sees_a_window_constant_off_by_1e_6 shows what that catches)."""
import os
import sys

import numpy as np
import pytest

import chan_grid_cases as cg
import test_chan_select_host as host

sys.path.insert(0, os.path.join(host.ROOT, "oracle"))
import orc_chan  # noqa: E402

FB_RATES = (1.0e6, 1.25e6, 2.0e6, 2.5e6, 4.0e6, 2.048e6, 1.92e6, 2.4e6)
RASTER = [(r * 10000.0, sps) for r in range(50, 801) for sps in range(1, 17)]


@pytest.fixture(scope="module", params=([], host.SAN), ids=("plain", "asan_ubsan"))
def exe(request, tmp_path_factory):
    return host._build(tmp_path_factory.mktemp("chan_plan"), request.param, "chan_plan_host")


def _f32(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def _vectors(out):
    """the program's "name count bits ..." lines -> {name: float32 array}"""
    vec = {}
    for ln in out.splitlines():
        w = ln.split()
        vec[w[0]] = _f32(w[2:])
        assert vec[w[0]].size == int(w[1]) * (2 if "bank" in w[0] or w[0] == "t1" else 1)
    return vec


def _taps(exe, which, fs, sps):
    return _vectors(host._run(exe, ["taps", which, "%.1f" % fs, str(sps)], ""))


def ulps(a, b):
    """distance of two float32 arrays in units in the last place (of the tap itself: neighbours on the float32 line are 1)"""
    def line(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(line(a) - line(b))


def same_taps(got, want):
    return got.size == want.size and bool(np.all(ulps(got, want) <= 1))


def test_the_tap_comparison_sees_a_window_constant_off_by_1e_6():
    want = orc_chan.firdes_low_pass(1.0, 2.0e6, 15625.0, 7812.5)
    assert same_taps(want, want)

    def mutated(gain, fs, cutoff, tw, a0=0.54 + 1e-6):
        ntaps = int(53.0 * fs / (22.0 * tw)) | 1
        M = (ntaps - 1) // 2
        n = np.arange(-M, M + 1, dtype=np.float64)
        w = a0 - 0.46 * np.cos(2.0 * np.pi * np.arange(ntaps) / (ntaps - 1))
        fw = 2.0 * np.pi * cutoff / fs
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(n == 0, fw / np.pi, np.sin(n * fw) / (n * np.pi)) * w
        return (t * (gain / (t[M] + 2.0 * t[M + 1:].sum()))).astype(np.float32)

    assert same_taps(mutated(1.0, 2.0e6, 15625.0, 7812.5, a0=0.54), want)          # the copy itself is the oracle's
    assert not same_taps(mutated(1.0, 2.0e6, 15625.0, 7812.5), want)


@pytest.fixture(scope="module")
def raster(exe):
    """the header's direct-mode plan of every raster cell: {(rate, sps): (ok, numbers, refusal text)}"""
    out = host._run(exe, ["ddc"], "".join("%.1f %d\n" % c for c in RASTER))
    rows = out.splitlines()
    assert len(rows) == len(RASTER)
    res = {}
    for c, ln in zip(RASTER, rows):
        head, _, text = ln.partition(" | ")
        w = head.split()
        res[c] = (w[0] == "ok", [int(v) for v in w[1:]], text)
    return res


def test_direct_mode_plans_over_the_10_khz_raster(raster):
    """0.5 .. 8 Msps by 10 kHz x sps 1 .. 16: decimations, step, taps per phase, resampler length and first filter are
    chan_grid_cases.direct_numbers'; the header refuses where that returns None and where the resampler's span does not fit
    (chan_grid_cases.plan_runs), and nowhere else"""
    span_refused = set()
    for (fs, sps), (ok, num, text) in raster.items():
        want = cg.direct_numbers(fs, sps)
        if want is None:
            assert not ok and "spans" not in text, (fs, sps, text)
            continue
        d1, d2, step, tpf, nt = want
        row = 30 if tpf <= 30 else 96
        assert num[:7] == [d1, d2, step.numerator, step.denominator, tpf, row, (nt // 2) % 32] and num[9] == nt, (fs, sps, num)
        runs = cg.plan_runs(step, row)
        assert ok == runs, (fs, sps, text)
        if not runs:
            assert text.startswith("ddc: %.1f samples/s at sps %d: the resampler" % (fs, sps)) and " spans " in text, text
            span_refused.add((fs, sps))
        else:
            assert text == ""
    assert set(host.REFUSED) <= span_refused and cg.DDC_SEARCH["long_refused"] in span_refused
    assert all(sps == 1 for _, sps in span_refused)
    for (fs, sps), span in host.REFUSED.items():
        assert "spans %d input samples per wave, the kernel's window holds 512" % span in raster[(fs, sps)][2]


def test_direct_mode_refusal_texts(exe):
    out = host._run(exe, ["ddc"], "2340000.0 4\n40000.0 4\n2000000.5 4\n").splitlines()
    assert out[0].endswith("| ddc: 2340000.0 is an exact multiple of 23400 x 4: the reference's own direct mode cannot run there "
                           "(_select_decim returns its factors without storing them, gmr1_rx_sdr.py:652-655)")
    assert out[1].endswith("| ddc: sample rate 40000.0 too low for a direct branch")
    assert out[2].endswith("| ddc: the sample rate must be a whole number of Hz")


@pytest.fixture(scope="module")
def fb_plans():
    return {fs: orc_chan.Plan(fs) for fs in FB_RATES}


def test_filterbank_plans_and_counts(exe, fb_plans):
    lengths = sorted(set(cg.short_lengths()) | {cg.N_GRID})
    cells = [(fs, sps, n) for fs in FB_RATES for sps in range(1, 17) for n in lengths]
    out = host._run(exe, ["chan"], "".join("%.1f %d %d\n" % c for c in cells)).splitlines()
    assert len(out) == len(cells)
    for (fs, sps, n), ln in zip(cells, out):
        w = ln.split(" | ")[0].split()
        assert w[0] == "ok", ln
        (n_chans, ntaps, n_blocks, tpf, j0, num, den, pre, pre_tpf, pre_j0, pre_num, pre_den, n_mid, T, n_out) = (int(v) for v in w[1:])
        pl = fb_plans[fs]
        st = cg.fb_step(sps)
        assert (n_chans, ntaps, n_blocks) == (pl.n_chans, pl.taps.size, -(-pl.taps.size // pl.n_chans) + 1), (fs, sps)
        assert (tpf, j0, num, den) == (-(-pl.taps_resamp.size // 32), cg.RRC_J0, st.numerator, st.denominator), (fs, sps)
        assert bool(pre) == (pl.pre_rate is not None)
        want_mid = n
        if pre:
            ps = cg.pre_step(fs)
            want_j0 = (pl.taps_pre.size // 2) % 32
            assert (pre_tpf, pre_j0, pre_num, pre_den) == (30, want_j0, ps.numerator, ps.denominator), fs
            want_mid = cg.resamp_count(ps, want_j0, n)
        want_T = want_mid // (pl.n_chans // 2)
        assert (n_mid, T, n_out) == (want_mid, want_T, cg.resamp_count(st, cg.RRC_J0, want_T)), (fs, sps, n)


def test_filterbank_refusals(exe):
    out = host._run(exe, ["chan"], "8100000.0 4 0\n2048000.5 4 0\n").splitlines()
    assert out[0].startswith("refused ") and out[0].endswith("| channelize: 260 channels (at most 256)")
    assert out[1].endswith("| channelize: the sample rate must be a whole number of Hz")


def test_filterbank_taps(exe, fb_plans):
    for fs in FB_RATES:
        pl = fb_plans[fs]
        v = _taps(exe, "chan", fs, 4)
        assert same_taps(v["taps"], pl.taps), fs
        assert same_taps(v["rrc"], pl.taps_resamp), fs
        if pl.pre_rate is not None:
            assert same_taps(v["pre_taps"], pl.taps_pre), fs
        else:
            assert v["pre_taps"].size == 0 and v["pre_bank"].size == 0


def test_direct_mode_taps(exe, raster):
    """the two low-passes and the root-raised cosine of every rate of the raster (they do not depend on sps), each distinct
    parameter set once"""
    seen = set()
    for r in range(50, 801):
        fs = r * 10000.0
        sps = next((s for s in range(1, 17) if raster[(fs, s)][0]), None)
        if sps is None:
            continue
        d1, d2 = raster[(fs, sps)][1][:2]
        key = {("lp1", d1), ("lp2", d2), ("rrc", fs / (d1 * d2))}
        if key <= seen:
            continue
        seen |= key
        pl = orc_chan.DirectPlan(fs, sps)
        v = _taps(exe, "ddc", fs, sps)
        assert same_taps(v["taps1"], pl.taps1), fs
        assert same_taps(v["taps2"], pl.taps2), fs
        assert same_taps(v["rrc"], pl.taps_resamp), fs


def _bank_rows(taps, row):
    """chan_grid_cases._banks in float32, its rows padded with zeros to `row` places, as (tap, difference) pairs"""
    b, d, tpf = cg._banks(taps, np.float32)
    out = np.zeros((32, row, 2), np.float32)
    out[:, :tpf, 0], out[:, :tpf, 1] = b, d
    return out


@pytest.mark.parametrize("which,fs,sps,row", (("chan", 2.0e6, 4, 30), ("chan", 2.048e6, 4, 30), ("ddc", 1.0e6, 2, 96),
                                              ("ddc", 2.0e6, 4, 30)))
def test_banks(exe, which, fs, sps, row):
    """every bank of an on-grid, an off-grid, a 96-tap and a padded 30-tap direct plan, from the plan's own taps: the zero
    padding and the last difference of 0 included"""
    v = _taps(exe, which, fs, sps)
    assert -(-v["rrc"].size // 32) <= row and (row == 96) == (-(-v["rrc"].size // 32) > 30)
    assert np.array_equal(v["bank"].reshape(32, row, 2), _bank_rows(v["rrc"], row))
    last = v["rrc"].size - 1
    assert v["bank"].reshape(32, row, 2)[last % 32, last // 32, 1] == 0.0
    if which == "chan" and fs == 2.048e6:
        assert np.array_equal(v["pre_bank"].reshape(32, 30, 2), _bank_rows(v["pre_taps"], 30))


def test_carrier_taps_and_rotation_step(exe):
    fs, sps, freqs = 2.0e6, 4, (94650.0, -218350.0)
    d1 = cg.direct_numbers(fs, sps)[0]
    taps1 = _taps(exe, "ddc", fs, sps)["taps1"]
    out = host._run(exe, ["carrier", "%.1f" % fs, str(sps)] + ["%.1f" % f for f in freqs], "").splitlines()
    t1 = _f32(out[0].split()[2:]).reshape(len(freqs), taps1.size, 2)
    rot = np.array([int(w, 16) for w in out[1].split()[2:]], np.uint64).view(np.float64)
    k = np.arange(taps1.size, dtype=np.float64)
    for c, f in enumerate(freqs):
        want = (taps1.astype(np.float64) * np.exp(2j * np.pi * f * k / fs)).astype(np.complex64)
        assert same_taps(t1[c, :, 0], want.real) and same_taps(t1[c, :, 1], want.imag), f
        assert rot[c] == (f / fs) * d1


def test_select_channels(exe):
    out = host._run(exe, ["select", "64", "5", "40", "31"], "").split()
    want = [-1] * 64
    want[5], want[40], want[31] = 0, 1, 2
    assert out[0] == "ok" and [int(v) for v in out[1:]] == want
    assert host._run(exe, ["select", "64", "5", "64"], "").strip() == "refused | channelize: channel index 64 outside 0..63"
    assert host._run(exe, ["select", "64", "5", "-1"], "").strip() == "refused | channelize: channel index -1 outside 0..63"
    assert host._run(exe, ["select", "64", "5", "40", "5"], "").strip() == "refused | channelize: channel 5 selected twice"
