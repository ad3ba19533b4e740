"""The oracle's fine FCCH acquisition and SNR estimate against the float64 restatement of tests/f64_fcch.py, over the whole
grid of tests/test_gpu_fcch_fine_grid.py and on the same inputs, on the CPU.

The product's contract (toa identical, freq_error within 1e-4 rad / symbol, SNR within 2e-4 relative)
is measured against the oracle.  It means something only if the oracle itself sits well inside those figures: here it has
to stay within a QUARTER of each of them of a computation that carries no fp32 rounding of its own, in every regime of the
grid -- all three burst types, 1 ... 16 samples per symbol, freq_shift absent, zero, small, what the receive loop passes and
0.95 pi rad / symbol.  The cases whose toa the restatement shows to be undecidable (f64_fcch.undecidable) are counted per
cell and capped at 2 %; the oracle alone has to meet that cap, which is what makes the GPU test's cap fair."""
import numpy as np
import pytest

import f64_fcch as F


@pytest.mark.parametrize("sps", F.SPS_GRID)
@pytest.mark.parametrize("which", list(F.TYPES))
def test_oracle_fine_and_snr_against_float64(orc, which, sps):
    worst_fe = worst_snr = 0.0
    for cls in F.SHIFT_CLASSES:
        cases = F.cell_cases(which, sps, cls)
        ref = F.f64_all(cases, sps, which)
        got = F.oracle_all(orc, cases, sps, which)
        left_out = 0
        for i, ((f, s), (rv, toa, fe, rv2, osnr)) in enumerate(zip(ref, got)):
            assert rv == 0 and rv2 == 0 and f["rv"] == 0
            why = F.undecidable(f)
            if why is None:
                assert toa == f["toa"], (which, sps, cls, i, toa, f)
            else:
                left_out += 1
            if why != "margin":
                worst_fe = max(worst_fe, abs(fe - f["freq_error"]))
                assert abs(fe - f["freq_error"]) <= F.TOL_FREQ / 4, (which, sps, cls, i, fe, f)
            worst_snr = max(worst_snr, abs(osnr - s) / max(1.0, abs(s)))
            assert abs(osnr - s) <= F.TOL_SNR / 4 * max(1.0, abs(s)), (which, sps, cls, i, osnr, s)
        assert left_out <= 0.02 * len(cases), (which, sps, cls, left_out)
    print("%s sps %d (%s): oracle - float64 worst |d freq_error| %.2e rad/symbol, worst rel |d snr| %.2e"
          % (which, sps, F.body_of(which, sps), worst_fe, worst_snr))


def test_restatement_finds_what_was_sent():
    """the restatement itself is no tautology: on clean bursts it returns the delay and the carrier offset that were put in
    (as far as the estimator does: a 5-bin centroid on a truncated chirp is some 15 % short or long in the delay)"""
    rng = np.random.default_rng(3)
    for which, (freq, n) in F.TYPES.items():
        for sps in (1, 4, 16):
            delay, cfo = 1.75 * sps, 400.0
            x = F.make_burst(rng, which, sps, None, cfo, delay, 0.0)
            f = F.fine(x, sps, None, which)
            assert abs(f["toa_samples"] - delay) < 0.3 * sps, (which, sps, f)
            assert abs(f["freq_error"] - 2 * np.pi * cfo / F.SYM_RATE) < 2e-3, (which, sps, f)
            # and a freq_shift of minus the estimate leaves (next to) nothing
            g = F.fine(x, sps, np.float32(-f["freq_error"]), which)
            assert abs(g["freq_error"]) < 2e-3 and abs(g["toa_samples"] - delay) < 0.3 * sps
            assert F.snr(x, sps, None, which)[1] > 10.0
    assert F.fine(np.zeros(100, np.complex64), 1)["rv"] == -22 and F.snr(np.zeros(100, np.complex64), 1)[0] == -22


def test_degenerate_windows_are_not_numbers(orc):
    """an all-zero window and a constant one take the sd == 0 branch and end in 0 / 0, in the oracle as in the restatement
    (the constant is dyadic and the window short enough that any summation order gives the mean exactly)"""
    for x in (np.zeros(117 * 2, np.complex64), np.full(117 * 2, 0.5 - 2.0j, np.complex64)):
        f = F.fine(x, 2)
        assert f["toa"] is None and np.isnan(f["freq_error"]) and np.isnan(F.snr(x, 2)[1])
        rv, _, fe = orc.fcch_fine(x, 2)
        assert rv == 0 and np.isnan(fe) and np.isnan(orc.fcch_snr(x, 2)[1])
