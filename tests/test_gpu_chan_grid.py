"""Every form of the arbitrary resampler against the numpy oracle (oracle/orc_chan.py), not only the one sps 4 runs: the
filterbank path at sps 1 .. 16, the generic filterbank and the pre-resampler in front of it, on-grid rotation, short captures
and the direct mode over its plans -- each sample under two bounds (chan_grid_cases: the 2e-4 contract and 8 x the float32
restatement's own distance from the float64 oracle; tests/test_chan_grid_host.py shows what the second one sees).  Which form
a cell runs is asserted from the rule (csrc/chan_select.h, restated in chan_grid_cases.resamp_form and held to the header by
tests/test_chan_select_host.py), and the module asserts that its cells reach every form.

One capture serves the filterbank cells: 661 237 samples at 2.0 Msps = 33 periods of the resampler and a ragged 34th, so a
wave's walk of 32 periods ends inside it and a second block exists; T = 20 663 is odd.  The direct mode's cells are at least one
whole period and a ragged second, 33 periods and a tail where that stays under 700 000 wideband samples (0.92, 1.0, 1.25
and 1.3 Msps); elsewhere the walk across blocks is the filterbank cells' job.

Run with -s for the measured ratio max|gpu - f64| / max|f32 - f64| of every cell (DESIGN 6 quotes the worst per family)."""
import numpy as np
import pytest

import chan_grid_cases as cg
import orc_chan

pytestmark = pytest.mark.gpu

FS = cg.FS


def _hold(name, got, ref, f32, rounding=True, envelope=0.0):
    """both bounds on one channel; -> the measured ratio.  envelope: a short capture's rounding scale is taken no smaller
    than the long cell's of the same signal, channel and sps (_short)"""
    assert got.size == ref.size, (name, got.size, ref.size)
    if ref.size == 0:
        return 0.0
    err = float(np.max(np.abs(got - ref)))
    contract, bound = cg.bounds(ref, f32 if f32 is not None else ref)
    bound = max(bound, cg.ROUNDING_FACTOR * envelope)
    ratio = err / (bound / cg.ROUNDING_FACTOR) if bound > 0 else (0.0 if err == 0 else float("inf"))
    print("%-44s err %.3e  contract %.1e  f32 %.3e  ratio %.2f" % (name, err, contract, bound / cg.ROUNDING_FACTOR, ratio))
    assert err < contract, (name, err, contract)
    if rounding:
        assert err <= bound, (name, err, bound, ratio)
    return ratio


def _tone_frequencies(got, tones, rate, skip):
    """the tones came out where they belong (analytic check of oracle and kernel alike): the periodogram's peak within 30 Hz.
    (The existing test's lag-one phase estimate is pulled towards zero by the channel's coloured noise -- by 0.8 % of the
    offset for the 0.5 tone, 30 to 33 Hz at 4 kHz depending on the window --; the peak is not.)"""
    for i, (k, f, a) in enumerate(tones):
        z = got[i][skip:].astype(np.complex128)
        assert rate / z.size < 10.0                          # bins of at most 10 Hz
        fest = np.fft.fftfreq(z.size, 1.0 / rate)[int(np.argmax(np.abs(np.fft.fft(z))))]
        assert abs(fest - f) < 30.0, (k, fest, f)
        assert abs(np.sqrt(np.mean(np.abs(z) ** 2)) - a) < 0.25 * a


def test_the_grid_reaches_every_form():
    assert cg.REQUIRED_FORMS <= cg.grid_forms(), cg.REQUIRED_FORMS - cg.grid_forms()


@pytest.mark.parametrize("sps", range(1, 17))
def test_filterbank_every_sps_matches_oracle(gpu_api, sps):
    x, pl, y64, _ = cg.fb_front()
    n_out, ref, r32 = cg.fb_cell(sps)
    f = cg.resamp_form(cg.fb_step(sps), 30, x.size // 32, n_out)
    assert (f["P"], f["Q"], f["span_r"] if f["per_lane"] == 2 else f["span"], f["form"]) == cg.FILTERBANK[sps]
    assert f["gz"] >= 2
    n_chans, n_mid, n_plan = gpu_api.channelize_plan(FS, sps, x.size)
    assert (n_chans, n_mid, n_plan) == (64, x.size // 32, n_out)
    got = gpu_api.channelize(x, FS, cg.CHANS, sps=sps)
    assert got.shape == (len(cg.CHANS), n_out)
    worst = max(_hold("filterbank sps %d %s ch %d" % (sps, f["form"], k), got[i], ref[k], r32[k]) for i, k in enumerate(cg.CHANS))
    print("filterbank sps %d %s: worst ratio %.2f" % (sps, f["form"], worst))
    _tone_frequencies(got, cg.tones(), orc_chan.SYM_RATE * sps, 500 * sps)


def _planar(api, t, n, fs, chans, sps, n_out, stride, rotation=0.0):
    import torch
    P = -(-len(chans) * stride // sps) + 2
    planes = torch.zeros((sps * P, 2), dtype=torch.float32, device="cuda")
    w = api.channelize_planar_dev(None, t.data_ptr(), n, fs, chans, planes.data_ptr(), stride, P, sps=sps, rotation=rotation)
    assert w == n_out
    torch.cuda.synchronize()
    b = planes.cpu().numpy().view(np.complex64).reshape(-1)
    g = np.arange(len(chans))[:, None] * stride + np.arange(n_out)[None, :]
    used = np.zeros(b.size, bool)
    used[(g % sps) * P + g // sps] = True
    assert not b[~used].any()                               # nothing written outside the streams' places
    return b[(g % sps) * P + g // sps]


@pytest.mark.parametrize("sps", range(1, 17))
def test_planar_equals_interleaved_bit_for_bit(gpu_api, sps):
    """k_resamp<30, 128 | 256, EXT> (the planar call) against the form the interleaved call runs -- for sps >= 4 the only test
    that k_resamp2 in each WG is k_resamp to the bit.  out_stride = n_out + 7 and three channels: n_sel x out_stride is no
    multiple of most sps."""
    import torch
    x = cg.fb_front()[0]
    n = x.size
    t = torch.from_numpy(x.view(np.float32).copy()).cuda()
    chans = [3, 60, 17]
    _, _, n_out = gpu_api.channelize_plan(FS, sps, n)
    stride = n_out + 7
    flat = torch.zeros((len(chans), stride, 2), dtype=torch.float32, device="cuda")
    assert gpu_api.channelize_dev(None, t.data_ptr(), n, FS, chans, flat.data_ptr(), stride, sps=sps) == n_out
    torch.cuda.synchronize()
    a = flat.cpu().numpy().view(np.complex64).reshape(len(chans), stride)
    b = _planar(gpu_api, t, n, FS, chans, sps, n_out, stride)
    assert not a[:, n_out:].any() and np.abs(a[:, :n_out]).max() > 0
    assert np.array_equal(b.view(np.uint32), a[:, :n_out].view(np.uint32))


@pytest.mark.parametrize("sps", [3, 5, 8, 10, 13, 16])
def test_streamed_equals_one_shot_bit_for_bit(gpu_api, sps):
    """six periods and a ragged tail in one random push schedule; one push is longer than the four periods a wave of the
    streamed form walks"""
    n = 6 * 20000 + 1237
    x = cg.fb_front()[0][:n]
    ref = gpu_api.channelize(x, FS, cg.CHANS, sps=sps)
    rng = np.random.default_rng(100 + sps)
    sizes = [0, 1, 31, 32, 33, 20013, 90017] + [int(v) for v in rng.integers(0, 3000, 12)]
    rng.shuffle(sizes)
    outs, pos = [], 0
    with gpu_api.ChanStream(FS, cg.CHANS, sps=sps) as cs:
        for k in sizes + [n]:
            k = min(k, n - pos)
            want = gpu_api.channelize_plan(FS, sps, pos + k)[2] - gpu_api.channelize_plan(FS, sps, pos)[2]
            assert cs.out_len(k) == want
            o = cs.push(x[pos:pos + k])
            assert o.shape == (len(cg.CHANS), want)
            outs.append(o)
            pos += k
    assert pos == n
    got = np.concatenate(outs, axis=1)
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("sps", cg.OTHER_SPS)
@pytest.mark.parametrize("fs,n", cg.OTHER_FRONT_ENDS)
def test_other_front_ends_match_oracle(gpu_api, fs, n, sps):
    """k_pfb_any (1.25 Msps, 40 channels) and the pre-resampler (2.048 Msps, 66 channels) in front of k_resamp<30,256>,
    <30,128> and k_resamp2<WG=8> on three work-groups, 33 periods and a tail"""
    x, pl, y64, _ = cg.fb_front(fs, n, 7)
    n_out, ref, r32 = cg.fb_cell(sps, fs, n, 7)
    chans = cg.chans_of(pl.n_chans)
    T = y64[chans[0]].size
    assert cg.resamp_form(cg.fb_step(sps), 30, T, n_out)["gz"] >= 2
    n_chans, n_mid, n_plan = gpu_api.channelize_plan(fs, sps, n)
    assert (n_chans, n_mid, n_plan) == (pl.n_chans, T, n_out)
    got = gpu_api.channelize(x, fs, chans, sps=sps)
    worst = max(_hold("%.3f Msps sps %d ch %d" % (fs / 1e6, sps, k), got[i], ref[k], r32[k]) for i, k in enumerate(chans))
    print("front end %.3f Msps sps %d: worst ratio %.2f" % (fs / 1e6, sps, worst))
    if pl.pre_rate is None:
        _tone_frequencies(got, cg.tones(pl.n_chans), orc_chan.SYM_RATE * sps, 500 * sps)


ROT_N = 200000 + 19


@pytest.mark.parametrize("fs,sps,planar", [(2.0e6, 1, False), (2.0e6, 1, True), (2.0e6, 4, False), (2.0e6, 4, True),
                                          (1.25e6, 4, False)])
def test_on_grid_rotation_matches_oracle(gpu_api, fs, sps, planar):
    """the filterbank's own pre-rotation (k_pfb64 / k_pfb_any <ROT>) against orc_chan.channelize(..., rotation=): one raster
    step as the C API takes it (a float) and one rotation unrelated to the raster.  The 2e-4 contract only: the device's fast
    sine is not the restatement's (measured worst, relative to the contract: see DESIGN 6)."""
    import torch
    pl = orc_chan.Plan(fs, sps)
    x = cg.capture(ROT_N, fs, 9, pl.n_chans)
    chans = cg.chans_of(pl.n_chans)
    _, _, n_out = gpu_api.channelize_plan(fs, sps, ROT_N)
    for rot in (float(np.float32(2 * np.pi * 31250.0 / fs)), float(np.float32(0.2137))):     # (the C API takes a float)
        ref = orc_chan.channelize(x, pl, chans, rotation=rot)
        if planar:
            t = torch.from_numpy(x.view(np.float32).copy()).cuda()
            got = _planar(gpu_api, t, ROT_N, fs, chans, sps, n_out, n_out + 7, rotation=rot)
        else:
            got = gpu_api.channelize(x, fs, chans, sps=sps, rotation=rot)
        for i, k in enumerate(chans):
            _hold("rotation %.4f %.2f Msps sps %d%s ch %d" % (rot, fs / 1e6, sps, " planar" if planar else "", k), got[i], ref[k],
                  None, rounding=False)


def _envelope(ref, r32):
    return {k: float(np.max(np.abs(r32[k] - ref[k]))) for k in ref}


def _short(api, x, fs, sps, n_in, chans, env):
    """One short capture, the head of a long cell's: counts, every output under both bounds, an untouched buffer where there
    is no output.  The rounding scale of a channel is the larger of the restatement's distance here and over the long cell
    (env): the outputs are the long cell's first ones (but for the last few, whose windows meet the stream's end), their
    errors draws from the same envelope, and the maximum of ten draws -- T = 29 at sps 1 -- does not estimate it: on the
    noise-only channels the restatement is 2.5e-9 from the oracle there and 4e-8 over the long cell, the product 6.6e-8 in
    both (its DFT stages round the tones' partial sums into every channel)."""
    import ctypes as C
    pl = orc_chan.Plan(fs, sps)
    D = pl.n_chans // 2
    T = n_in // D
    n_out = cg.resamp_count(cg.fb_step(sps), cg.RRC_J0, T)
    assert api.channelize_plan(fs, sps, n_in) == (pl.n_chans, T, n_out)
    xs = np.ascontiguousarray(x[:max(n_in, 1)])
    ch = np.asarray(chans, np.int32)
    out = np.full((len(chans), n_out + 3), np.complex64(complex(7.5, -3.25)))
    got_n = C.c_uint64(99)
    lib = api.load()
    rc = lib.gmr1_hip_channelize(C.c_double(fs), C.c_int(sps), xs.ctypes.data_as(C.c_void_p), C.c_uint64(n_in), C.c_float(0.0),
                                 C.c_int(len(chans)), ch.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                 C.c_uint64(n_out + 3), C.byref(got_n))
    assert rc == 0 and got_n.value == n_out, (fs, sps, n_in, rc, got_n.value, n_out)
    if n_out == 0:
        assert (out == np.complex64(complex(7.5, -3.25))).all()
        return 0.0
    y64 = orc_chan.pfb_channelizer_2x(x[:n_in], pl.taps, pl.n_chans)
    y32 = cg.pfb_f32(x[:n_in], pl.taps, pl.n_chans)
    worst = 0.0
    for i, k in enumerate(chans):
        ref = cg.resample(y64[k], cg.fb_step(sps), pl.taps_resamp, n_out)
        assert np.array_equal(ref, orc_chan.arb_resampler(y64[k], pl.resamp, pl.taps_resamp, 32))
        r32 = cg.resample(y32[k], cg.fb_step(sps), pl.taps_resamp, n_out, f32=True)
        worst = max(worst, _hold("short %.2f Msps sps %d n_in %d ch %d" % (fs / 1e6, sps, n_in, k), out[i, :n_out], ref, r32,
                                 envelope=env[k]))
    return worst


@pytest.mark.parametrize("sps", cg.SHORT_SPS)
def test_short_captures_filterbank(gpu_api, sps):
    """T = n_in // 32 = 0, 1, 2, 3, 29 .. 31, 63 .. 65, 127 .. 129, 160: the switch of forms at T < 2, windows of 128 samples
    clamped to and repaired at the ends of streams shorter than they are, the filterbank's eleven blocks of history"""
    x = cg.fb_front()[0]
    env = _envelope(*cg.fb_cell(sps)[1:])
    worst = max(_short(gpu_api, x, FS, sps, n_in, cg.CHANS, env) for n_in in cg.short_lengths())
    print("short captures 2.0 Msps sps %d: worst ratio %.2f" % (sps, worst))


@pytest.mark.parametrize("sps", cg.SHORT_SPS)
def test_short_captures_generic_filterbank(gpu_api, sps):
    fs, n = cg.OTHER_FRONT_ENDS[0]
    x = cg.fb_front(fs, n, 7)[0]
    env = _envelope(*cg.fb_cell(sps, fs, n, 7)[1:])
    worst = max(_short(gpu_api, x, fs, sps, 20 * T + (11 if T else 0), cg.chans_of(40), env) for T in cg.SHORT_ANY_T)
    print("short captures 1.25 Msps sps %d: worst ratio %.2f" % (sps, worst))


@pytest.mark.parametrize("sps", cg.SHORT_SPS)
def test_short_captures_direct(gpu_api, sps):
    """2.0 Msps, decimation 7 x 6: 41 / 42 and 83 / 84 samples are either side of the first and second stage-2 output"""
    d = cg.Direct(FS, sps)
    x, _, ref_long, r32_long = cg.ddc_cell(FS, sps)          # the heads of the long cell, its envelope as in _short
    env = [float(np.max(np.abs(a - b))) for a, b in zip(r32_long, ref_long)]
    worst = 0.0
    for n_in in cg.SHORT_DDC_N:
        n_out = d.n_out(n_in)
        assert gpu_api.ddc_plan(FS, sps, n_in)[3] == n_out
        got = gpu_api.ddc(x[:n_in], FS, cg.DDC_FREQS, sps=sps)
        assert got.shape == (3, n_out)
        T = n_in // d.d1 // d.d2
        if n_out == 0:
            continue
        for i, f in enumerate(cg.DDC_FREQS):
            ref = cg.resample(cg.ddc_stages(x[:n_in], d, f)[:T], d.step, d.pl.taps_resamp, n_out)
            r32 = cg.resample(cg.ddc_stages(x[:n_in], d, f, f32=True)[:T], d.step, d.pl.taps_resamp, n_out, f32=True)
            worst = max(worst, _hold("short direct sps %d n_in %d carrier %d" % (sps, n_in, i), got[i], ref, r32,
                                     envelope=env[i]))
    print("short captures direct sps %d: worst ratio %.2f" % (sps, worst))


@pytest.mark.parametrize("fs,sps", cg.ddc_cells(), ids=lambda v: str(v))
def test_direct_mode_every_form_matches_oracle(gpu_api, fs, sps):
    d = cg.Direct(fs, sps)
    if not d.runs:
        # refused by the plan, the one-shot call and the stream alike, before anything is launched
        x = np.zeros(4096, np.complex64)
        for call in (lambda: gpu_api.ddc_plan(fs, sps, 100000), lambda: gpu_api.ddc(x, fs, cg.DDC_FREQS, sps=sps),
                     lambda: gpu_api.ChanStream.direct(fs, cg.DDC_FREQS, sps=sps)):
            with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
                call()
        return
    x, n_out, ref, r32 = cg.ddc_cell(fs, sps)
    f = d.form(x.size)
    d1, d2, rs, n_plan = gpu_api.ddc_plan(fs, sps, x.size)
    assert (d1, d2, n_plan) == (d.d1, d.d2, n_out) and abs(rs - d.pl.resamp) < 1e-12
    got = gpu_api.ddc(x, fs, cg.DDC_FREQS, sps=sps)
    assert got.shape == (3, n_out)
    worst = max(_hold("direct %.2f Msps sps %d %s carrier %d" % (fs / 1e6, sps, f["form"], i), got[i], ref[i], r32[i])
                for i in range(3))
    print("direct %.2f Msps sps %d %s: worst ratio %.2f" % (fs / 1e6, sps, f["form"], worst))
    for i in range(3):
        z = got[i][min(1000 * sps, n_out // 2):].astype(np.complex128)
        fest = np.angle(np.mean(z[1:] * np.conj(z[:-1]))) / (2 * np.pi) * orc_chan.SYM_RATE * sps
        assert abs(fest - 900.0) < 40.0, (fs, sps, i, fest)
    with gpu_api.ChanStream.direct(fs, cg.DDC_FREQS, sps=sps) as cs:
        assert cs.out_len(x.size) == n_out
