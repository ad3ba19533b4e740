"""That the channelizer grid's rounding-scale bound means something, without a GPU (tests/test_gpu_chan_grid.py holds the
product to it): on each cell's own input, five mutations of the float64 reference -- the resampler prototype's last tap
dropped, its first tap dropped, the derivative term dropped, the fraction taken from the next output, the filter index off
by one on every 64th output -- must each move at least one compared sample of every compared channel by more than 10 times
that cell's bound (8 x the largest difference between the float32 restatement and the float64 oracle on that channel).  The
contract bound 2e-4 max(1, rms) sees none of the first two on the noise-only channels.  Also: the helper's float64 form is
the oracle's bit for bit, the short captures' counts, and the grid's form coverage from the rule alone."""
import numpy as np
import pytest

import chan_grid_cases as cg
import orc_chan

MUT_OUTPUTS = 20000            # outputs a mutation is evaluated over: "at least one sample" needs no more


def _mutations_exceed(name, y64, step, taps, ref, f32):
    n = min(ref.size, MUT_OUTPUTS)
    contract, bound = cg.bounds(ref, f32)
    assert 0 < bound < contract / 20, (name, bound, contract)      # the second bound is the tight one
    for mut in cg.MUTATIONS:
        moved = float(np.max(np.abs(cg.resample(y64, step, taps, n, mut=mut) - ref[:n])))
        assert moved > cg.MUTATION_FACTOR * bound, (name, mut, moved, bound)
    return bound


@pytest.mark.parametrize("sps", range(1, 17))
def test_filterbank_cells_mutations_exceed_the_rounding_bound(sps):
    x, pl, y64, y32 = cg.fb_front()
    n_out, ref, r32 = cg.fb_cell(sps)
    st = cg.fb_step(sps)
    f = cg.resamp_form(st, 30, y64[5].size, n_out)
    assert (f["P"], f["Q"], f["span_r"] if f["per_lane"] == 2 else f["span"], f["form"]) == cg.FILTERBANK[sps]
    assert f["gz"] >= 2                                            # a second block of 32 periods exists
    # the helper's float64 form is the oracle's
    o = orc_chan.channelize(x, orc_chan.Plan(cg.FS, sps), [5])[5]
    assert o.size == n_out and np.array_equal(o, ref[5])
    for k in cg.CHANS:
        _mutations_exceed((sps, k), y64[k], st, pl.taps_resamp, ref[k], r32[k])


def test_end_taps_are_invisible_to_the_contract_bound_on_noise_channels():
    """why a second bound: a dropped end tap of the resampler's prototype stays under 2e-4 on the channels that carry noise
    only"""
    x, pl, y64, y32 = cg.fb_front()
    n_out, ref, r32 = cg.fb_cell(4)
    for k in (0, 63, 32):
        for mut in ("last_tap", "first_tap"):
            moved = float(np.max(np.abs(cg.resample(y64[k], cg.fb_step(4), pl.taps_resamp, n_out, mut=mut) - ref[k])))
            assert moved < cg.CONTRACT, (k, mut, moved)


@pytest.mark.parametrize("fs,sps", cg.ddc_cells(), ids=lambda v: str(v))
def test_direct_cells_mutations_exceed_the_rounding_bound(fs, sps):
    d = cg.Direct(fs, sps)
    if not d.runs:
        assert (fs, sps) in ((1.0e6, 1), cg.DDC_SEARCH["long_refused"])
        return
    x, n_out, ref, r32 = cg.ddc_cell(fs, sps)
    f = d.form(x.size)
    assert n_out > f["P"] and (n_out > 33 * f["P"] or 33 * f["Q"] * d.d1 * d.d2 >= 700000)
    o = orc_chan.direct_ddc(x, d.pl, cg.DDC_FREQS[1], n_out=n_out)
    assert np.array_equal(o, ref[1])
    _, y64, _ = cg.ddc_front(fs, cg.ddc_rate_length(fs))
    T = x.size // d.d1 // d.d2
    for i in range(len(cg.DDC_FREQS)):
        _mutations_exceed((fs, sps, i), y64[i][:T], d.step, d.pl.taps_resamp, ref[i], r32[i])


def test_short_capture_counts():
    """T = n_in // 32 channel samples, ((32 T - 22) den) // num outputs: none before the first filter's phase is reached"""
    want_T = [0, 0] + [T for T in cg.SHORT_T if T]
    assert [n // 32 for n in cg.short_lengths()] == want_T
    # by hand: 32 T - 22 thirty-seconds of an input sample are available, an output costs 2 000 000 / (23 400 sps) of them
    by_hand = {1: {1: 0, 2: 0, 3: 0, 29: 10, 129: 48, 160: 59}, 4: {1: 0, 2: 1, 3: 3, 29: 42, 129: 192, 160: 238},
               16: {1: 1, 2: 7, 3: 13, 29: 169, 129: 768, 160: 954}}
    for sps in cg.SHORT_SPS:
        st = cg.fb_step(sps)
        for T in want_T:
            n = cg.resamp_count(st, cg.RRC_J0, T)
            assert n == max(0, ((32 * T - 22) * 234 * sps) // 20000)
            if T in by_hand[sps]:
                assert n == by_hand[sps][T], (sps, T, n)
            f = cg.resamp_form(st, 30, T, n)
            # T < 2 keeps one output per lane whatever the plan
            assert f["form"] == "none" if n == 0 else (T >= 2 or f["per_lane"] == 1)
    assert cg.resamp_count(cg.fb_step(4), cg.RRC_J0, 0) == 0


def test_the_grid_reaches_every_form():
    assert cg.REQUIRED_FORMS <= cg.grid_forms(), cg.REQUIRED_FORMS - cg.grid_forms()
