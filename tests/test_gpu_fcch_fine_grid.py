"""k_fcch_fine (gmr1_fcch_fine and gmr1_fcch_snr, fcch_kernels.hip) against the oracle over its whole argument grid.

tests/test_gpu_fcch.py runs the kernel at 4 samples per symbol without a freq_shift.  The receive loop calls it with one
(-freq_err, and -(freq_err + fine's own estimate), gmr1_rx.c:682 / :694) at every sps.  Here, per burst type (fcch,
fcch3_lband, fcch3_sband) and sps (1, 2, 3, 4, 5, 8, 16), 5 shift classes x 50 bursts:

    none    no freq_shift array at all           zero    0.0 passed explicitly
    small   +-0.02 rad / symbol                  loop    minus the fine estimate of that burst (carrier 100 ... 2000 Hz off)
    edge    +-0.95 pi rad / symbol: the burst comes out 0.95 pi off, at the end of what fine can return

at 0, 3, 6, 10, 20 dB and noiseless, delayed by up to +-3 symbols (a real number of samples), every other window on a DC
offset, all windows of a (type, sps) in ONE flat array at odd offsets that are no multiples of sps, the gaps filled with a
value far above the signal.  The four classes that carry a freq_shift go through one batch of 200 with their values mixed;
"none" is a batch of 50; batches of 1 and 2 and the reference's single calls (the shift as a C float) repeat part of them.

Which of the kernel's two bodies a (type, sps) reaches (nraw = len * sps <= 512: windows held in registers, the last
register partly masked unless nraw is 512; otherwise the loop over memory):

    fcch (117)          sps 1, 2, 3, 4: registers (117, 234, 351, 468 of 512 slots)     sps 5, 8, 16: memory
    fcch3_* (468)       sps 1: registers (468 of 512)                                    sps 2 ... 16: memory

Contract (unchanged for the new regimes): toa identical, freq_error within 1e-4 rad / symbol, SNR
within 2e-4 relative.  tests/test_fcch_f64_host.py shows on the same inputs that the oracle stays within a quarter of each
figure of a float64 restatement (worst seen: 1.5e-6 rad / symbol, 1.1e-5 relative), so none of them rests on the oracle's
own rounding.

A case is left out of the toa comparison only where the float64 restatement (tests/f64_fcch.py) shows it undecidable:
its best 5-bin window leads the best non-overlapping one by less than 1e-3 relative, or its continuous toa_samples lies
within f64_fcch.HALF_DELTA of a half-integer.  HALF_DELTA is four times what was measured: f64_fcch.measure_half_delta
(seed 20261: 20 000 random bursts across the grid plus bursts steered onto a half-integer and stepped across it in a
ladder from 1e-7 to 4e-3 samples) compared the oracle's integer with the restatement's and recorded the largest distance
from a half-integer at which they differ: 6.352e-4 samples (866 disagreements in 28 820 bursts compared, none further out;
f64_fcch.HALF_DELTA_MEASURED), so HALF_DELTA is 2.54e-3.  At most 2 % of a cell (one case of 50) may be left out, asserted;
such a case keeps its freq_error comparison unless it is the window margin that fails.  With the grid's seed, 22 of the 105
cells leave out one case each (all for the half-integer, none for the margin) and 83 none: 5 228 of 5 250 toa compared.
"""
import numpy as np
import pytest

import f64_fcch as F

pytestmark = pytest.mark.gpu


def _check(tag, f, o, toa, fe, snr, counts):
    """one burst: product (toa, fe, snr) against the oracle's o = (rv, toa, fe, rv, snr); f is the restatement's view"""
    assert o[0] == 0 and o[3] == 0, tag
    why = F.undecidable(f)
    counts[why] = counts.get(why, 0) + 1
    if why is None:
        assert toa == o[1], (tag, toa, o[1], f)
    if why != "margin":
        assert abs(fe - o[2]) < F.TOL_FREQ, (tag, fe, o[2], f)
    assert abs(snr - o[4]) <= F.TOL_SNR * max(1.0, abs(o[4])), (tag, snr, o[4])


@pytest.mark.parametrize("sps", F.SPS_GRID)
@pytest.mark.parametrize("which", list(F.TYPES))
def test_fine_and_snr_grid(gpu_api, orc, which, sps):
    cells = {cls: F.cell_cases(which, sps, cls) for cls in F.SHIFT_CLASSES}
    want = {cls: F.oracle_all(orc, cells[cls], sps, which) for cls in F.SHIFT_CLASSES}
    ref = {cls: [F.fine(c["x"], sps, c["fs"], which) for c in cells[cls]] for cls in F.SHIFT_CLASSES}
    report = []
    # ---- "none": a batch of its own, freq_shift = NULL
    # ---- the rest: one batch of 200, the classes interleaved so that neighbours carry different shifts
    shifted = [cls for cls in F.SHIFT_CLASSES if cls != "none"]
    mixed = [(cls, i) for i in range(F.CELL) for cls in shifted]
    for name, members in (("none", [("none", i) for i in range(F.CELL)]), ("mixed", mixed)):
        cases = [cells[cls][i] for cls, i in members]
        iq, offset = F.flat_layout(cases, sps)
        assert all(int(o) % 2 == 1 and (sps == 1 or int(o) % sps) for o in offset)
        fs = None if name == "none" else np.array([c["fs"] for c in cases], np.float32)
        toa, fe = gpu_api.fcch_fine_batch(iq, offset, sps=sps, freq_shift=fs, fcch_type=which)
        snr = gpu_api.fcch_snr_batch(iq, offset, sps=sps, freq_shift=fs, fcch_type=which)
        counts = {cls: {} for cls in F.SHIFT_CLASSES}
        for k, (cls, i) in enumerate(members):
            _check((which, sps, cls, i), ref[cls][i], want[cls][i], toa[k], fe[k], snr[k], counts[cls])
        for cls in sorted({m[0] for m in members}):
            out = F.CELL - counts[cls].get(None, 0)
            assert out <= 0.02 * F.CELL, (which, sps, cls, counts[cls])
            report.append("%s %d/%d" % (cls, out, F.CELL))
        # ---- batches of 1 and of 2 from the same array (the second burst of the two: a different shift)
        for nb in (1, 2):
            t2, f2 = gpu_api.fcch_fine_batch(iq, offset[:nb], sps=sps, freq_shift=None if fs is None else fs[:nb],
                                             fcch_type=which)
            s2 = gpu_api.fcch_snr_batch(iq, offset[:nb], sps=sps, freq_shift=None if fs is None else fs[:nb],
                                        fcch_type=which)
            assert np.array_equal(t2, toa[:nb]) and np.array_equal(f2, fe[:nb]) and np.array_equal(s2, snr[:nb])
    # ---- the reference's single calls, the shift as the C float of the argument list: four bursts of every class
    for cls in F.SHIFT_CLASSES:
        for i in range(0, F.CELL, 13):
            c = cells[cls][i]
            shift = 0.0 if c["fs"] is None else float(c["fs"])
            rv, t, f = gpu_api.fcch_fine(c["x"], sps, shift, which)
            rv2, s = gpu_api.fcch_snr(c["x"], sps, shift, which)
            assert rv == 0 and rv2 == 0
            _check((which, sps, cls, i, "single"), ref[cls][i], want[cls][i], t, f, s, {})
    print("%s sps %d, %s body; left out of the toa comparison: %s" % (which, sps, F.body_of(which, sps), ", ".join(report)))


@pytest.mark.parametrize("which", list(F.TYPES))
def test_degenerate_windows(gpu_api, orc, which):
    """An all-zero window and a constant one: the deviation is 0, sd == 0 takes its branch (sd = 1), every bin is 0 and
    both centroids and the SNR are 0 / 0.  Whatever the oracle returns for that is what the product returns: the same rv,
    the same toa, and not-a-number where the oracle has not-a-number.  (The constants are dyadic and the sums stay far
    below 2^24 of their unit: the mean is exact in any order of summation, in fp32 as in float64.)  A live burst before
    and after them in the same batch is untouched."""
    n = F.TYPES[which][1]
    rng = np.random.default_rng(77)
    for sps in (1, 3, 4, 8):
        live = F.make_burst(rng, which, sps, 10.0, 300.0, 1.25 * sps, 0.0)
        cases = [dict(x=live), dict(x=np.zeros(n * sps, np.complex64)), dict(x=np.full(n * sps, 0.5 - 2.0j, np.complex64)),
                 dict(x=np.full(n * sps, -3.0 + 0.0j, np.complex64)), dict(x=live)]
        iq, offset = F.flat_layout(cases, sps)
        for fs in (None, np.array([0.02, -0.3, 0.02, 1.5, 0.02], np.float32)):
            toa, fe = gpu_api.fcch_fine_batch(iq, offset, sps=sps, freq_shift=fs, fcch_type=which)
            snr = gpu_api.fcch_snr_batch(iq, offset, sps=sps, freq_shift=fs, fcch_type=which)
            for k, c in enumerate(cases):
                shift = 0.0 if fs is None else float(fs[k])
                rv, otoa, ofe = orc.fcch_fine(c["x"], sps, shift, which=which)
                rv2, osnr = orc.fcch_snr(c["x"], sps, shift, which=which)
                assert rv == 0 and rv2 == 0
                tag = (which, sps, k, shift)
                assert toa[k] == otoa, (tag, toa[k], otoa)
                if k in (0, 4):
                    assert abs(fe[k] - ofe) < F.TOL_FREQ and abs(snr[k] - osnr) <= F.TOL_SNR * max(1.0, abs(osnr)), tag
                else:
                    assert np.isnan(ofe) and np.isnan(osnr), (tag, ofe, osnr)
                    assert np.isnan(fe[k]) and np.isnan(snr[k]), (tag, fe[k], snr[k])
                    single = gpu_api.fcch_fine(c["x"], sps, shift, which)
                    assert single[0] == 0 and single[1] == otoa and np.isnan(single[2]), (tag, single)
                    assert np.isnan(gpu_api.fcch_snr(c["x"], sps, shift, which)[1]), tag
