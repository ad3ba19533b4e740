"""The four-bursts-per-wave demodulator (k_rx4g, rx_kernels.hip) against the oracle on every format it takes, at every window
width at which its shape changes, every burst compared -- tests/test_gpu_demod_grid.py's rules, on the kernel a caller gets
at scale: every gmr1_hip_demod_batch* call of more than 4096 bursts at 4 samples per symbol, and gmr1_hip_tch3_rx_batch*
through k_rx4g_tch3.

The cells (demod4_cases.CELLS; in_len = len * 4 + extra, extra + 1 lags):

    k_rx4g<8,4>       nt3_speech +1 +6 +15 +16 +31 +32 +40      dc2 +12 +36
    k_rx4g<16,4>      nt3_speech +41 +104    dc2 +37 +100       bcch +1 +16 +80 +84     dc6 +1 +40 +63 +64 +88
    k_rx4g<8,4,true>  nt3_facch +1 +6 +15 +16 +32
    k_rx (n > 4096)   bcch +85               dc2 +101           nt3_facch +33

The widths are where cw = (lags + 15) & ~15, which carves the LDS, steps (16 / 17, 32 / 33, 64 / 65 lags), where the small
variant's staging is full (64 samples), where the small formats leave it for the generic variant (one chunk, 78 or 117
symbols in a kernel unrolled for three and 256), and the limits of demod_kernel_choice (rx_select.h) with one step past
each.  Batches of 4097, 4098 or 4099 bursts (one of 4100): the last wave holds 1, 2 or 3.

Per cell (demod4_cases.cell_inputs): a quarter of the bursts at lags 0 or 1, a quarter at the last two lags, the rest
anywhere, a fraction of a sample each, carrier offsets of 150 Hz rms, Es/N0 15 dB; a fifth with a constant offset of the
burst's own amplitude (the small variant forms its variance as sum |x|^2 - n |mean|^2); all-zero windows at each place of a
wave, a whole wave of them, a constant window, the batch's last burst; the windows scattered over one array at every
alignment, 1e6 between them and nothing behind the last one (the kernel fetches the next burst's window ahead).
Demodulated with the shift that takes the offset out and with an unrelated one.

Asserted on EVERY burst: rv == oracle's, sync_id == oracle's, toa within 16 / 1024; on every SAFE
burst -- the oracle's toa more than 32 / 1024 from the nearest x.5, decided from the oracle alone -- freq_err to 1e-5, all
soft symbols to 1e-4 on the circle, all soft bits to 1 LSB but for _compare_ebits' midpoint exceptions, whose number is
held to max(1, 2e-5 * bits).  Windows without a burst: rv = -1 and zeros.  The same batch in calls of at most 4096 bursts
(k_rx) gives the same decisions and, per burst, the same soft symbols and bits."""
import numpy as np
import pytest

import demod4_cases as d4
from demod4_cases import CELLS, KINDS, ONE_LAG, STRIDED, TCH3, cell_id, cell_inputs, check_inputs
from test_gpu_demod_grid import FORMATS, TOA_TOL, _compare_ebits, _compare_full
from test_rx_select_host import BUILDS, run_rx_select_host

gpu = pytest.mark.gpu
OUTPUTS = ("rv", "sync_id", "toa", "freq_err", "ebits", "ssyms")


# ---- host: the table against the rule, the inputs against the oracle ------------------------------------------------------
@BUILDS
def test_cells_get_the_kernel_the_table_says(tmp_path, extra):
    """On a GPU a wrong kernel choice is invisible, so demod_kernel_choice itself (tests/c/rx_select_host.cpp, handed the
    cells) says which kernel each cell's call gets and what it stages; the grid reaches all three k_rx4g instantiations
    and k_rx"""
    cells = CELLS + ONE_LAG
    args = ["%d:%d:%d" % (FORMATS.index(name), ext, d4.batch_size((impl, name, ext))) for impl, name, ext in cells]
    lines = run_rx_select_host(tmp_path, extra, args)
    assert len(lines) == len(cells)
    for (impl, name, ext), line in zip(cells, lines):
        t, e, n, got_impl, stage = (int(x) for x in line.split())
        assert (t, e, n) == (FORMATS.index(name), ext, d4.batch_size((impl, name, ext)))
        assert got_impl == impl, (name, ext, "the rule gives impl", got_impl, "the table says", impl)
        assert (stage > 0) == (impl != 0)
        if (name, ext) in d4.STAGE:
            assert stage == d4.STAGE[(name, ext)], (name, ext, stage)
    assert {c[0] for c in CELLS} == {0, 2, 3, 4} and {c[0] for c in ONE_LAG} == {2, 3, 4}
    assert len(CELLS) == 30 and len(set(CELLS)) == 30 and d4.BIG in CELLS
    assert {d4.batch_size(c) for c in CELLS} == {4097, 4098, 4099, 4100}
    for impl in (2, 3, 4):
        assert {d4.batch_size(c) % 4 for c in CELLS if c[0] == impl} >= {1, 2, 3}
    for group in (STRIDED, TCH3):
        assert all(c in CELLS for c in group)
    assert [c[0] for c in STRIDED] == [3, 2, 4] and [c[0] for c in TCH3] == [3, 3, 3, 3, 2]


def test_grid4_inputs_on_the_oracle(orc, pkg):
    """What the GPU tests below rest on holds with the oracle alone (demod4_cases.check_inputs)"""
    st = {cell: check_inputs(cell_inputs(pkg, orc, cell)) for cell in CELLS}
    print("share of safe bursts: %.3f ... %.3f" % (min(s["safe"] for s in st.values()), max(s["safe"] for s in st.values())))
    bers = [s["ber"] for s in st.values() if s["ber"] is not None]
    print("the oracle's bit error rate with the matching shift: %.4f ... %.4f" % (min(bers), max(bers)))
    for cell in ONE_LAG:
        c = cell_inputs(pkg, orc, cell)
        for kind in KINDS:
            assert (c["ref"][kind].rv == -1).all()


# ---- the comparison -------------------------------------------------------------------------------------------------------
def _demod(gpu_api, c, fs, rows=None):
    off = c["offset"] if rows is None else c["offset"][rows]
    fs = fs if fs is None or rows is None else fs[rows]
    return gpu_api.demod_batch(c["name"], c["iq"], off, c["in_len"], sps=c["sps"], freq_shift=fs)


def _check(c, kind, got, full=True, misses=None):
    """got (a call's answer to c's windows with the shifts of `kind`) against the oracle by the module's rules -> dict(safe,
    compared, mid: midpoint exceptions, ssym / freq_err: the largest distances among the safe bursts).  full=False: the
    call has no freq_err and no soft symbols (gmr1_hip_tch3_rx_batch), and its soft bits are compared alone.  Soft symbols
    beyond the tolerance fail here, or go to the caller's list `misses`, which then asserts that it is empty."""
    fmt, ref, safe = c["fmt"], c["ref"][kind], c["safe"][kind]
    n = c["n"]
    rv_differ = np.nonzero(got["rv"] != ref.rv)[0]
    assert rv_differ.size == 0, (cell_id(c["cell"]), kind, "rv", rv_differ[:8], got["rv"][rv_differ[:8]], ref.rv[rv_differ[:8]])
    st = dict(safe=int(safe.sum()), compared=0, mid=0, ssym=0.0, freq_err=0.0)
    own = misses is None
    misses = [] if own else misses
    for i in range(n):
        tag = (cell_id(c["cell"]), kind, "burst", i, "place", i % 4, "sent at lag", int(c["lag"][i]), "offset" if c["dc"][i] else "")
        if ref.rv[i] != 0:
            # no burst in the window: nothing comes out
            assert ref.rv[i] == -1 and i in c["silent"], tag
            for k in ("toa", "freq_err", "ebits", "ssyms") if full else ("toa", "ebits"):
                assert not np.any(got[k][i]), (tag, k, got[k][i])
            continue
        assert got["sync_id"][i] == ref.sync_id[i], (tag, "sync_id", got["sync_id"][i], ref.sync_id[i])
        assert abs(float(got["toa"][i]) - ref.toa[i]) < TOA_TOL, (tag, "toa", got["toa"][i], ref.toa[i])
        if not safe[i]:
            continue
        o = ref[i]
        if full:
            st["mid"] += _compare_full(c, got, i, o, tag, misses)
            d = np.abs(got["ssyms"][i].astype(np.float64) - o["ssyms"])
            st["ssym"] = max(st["ssym"], float(np.minimum(d, np.abs(d - 2.0 ** fmt.nbits)).max()))
            st["freq_err"] = max(st["freq_err"], abs(float(got["freq_err"][i]) - o["freq_err"]))
        else:
            st["mid"] += _compare_ebits(c, got["ebits"][i], o, tag)
        st["compared"] += 1
    assert not (own and misses), ("%d soft symbols differ by 1e-4 or more" % len(misses), misses[:8])
    bits = st["compared"] * fmt.ebits
    assert st["mid"] <= max(1, int(2e-5 * bits)), (cell_id(c["cell"]), kind, "%d midpoint symbols in %d soft bits" % (st["mid"], bits))
    return st


def _same_as_one_per_wave(c, kind, big, parts):
    """the one call (k_rx4g) against the same bursts in calls of at most 4096 (k_rx), burst by burst"""
    fmt, tag = c["fmt"], (cell_id(c["cell"]), kind, "one call against calls of at most 4096 bursts")
    small = {k: np.concatenate([p[k] for p in parts]) for k in OUTPUTS}
    assert np.array_equal(big["rv"], small["rv"]) and np.array_equal(big["sync_id"], small["sync_id"]), tag
    assert np.abs(big["toa"].astype(np.float64) - small["toa"]).max() <= TOA_TOL, tag
    same = np.nonzero(np.rint(big["toa"]) == np.rint(small["toa"]))[0]
    d = np.abs(big["ssyms"][same].astype(np.float64) - small["ssyms"][same])
    d = np.minimum(d, np.abs(d - 2.0 ** fmt.nbits)).max(axis=1)
    assert (d < 1e-4).all(), (tag, "soft symbols of bursts", same[~(d < 1e-4)][:8], d[~(d < 1e-4)][:8])
    deb = np.abs(big["ebits"][same].astype(int) - small["ebits"][same].astype(int)).max(axis=1)
    mid = 0
    for i in same[deb > 1]:
        mid += _compare_ebits(c, big["ebits"][i], dict(ebits=small["ebits"][i], ssyms=small["ssyms"][i]), tag + ("burst", int(i)))
    return dict(same_pick=int(same.size), mid=mid)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _halves(n):
    return [np.arange(0, n // 2), np.arange(n // 2, n)]


@gpu
@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_demod4_grid(gpu_api, orc, pkg, cell):
    """What this grid found in the kernels' stores is held by test_strided_rows_and_absent_outputs below; what it found in the
    soft symbols is held here.  With the constant offset, 16 soft symbols of the 17.4 million compared per shift were
    1.00e-4 ... 5.07e-4 from the oracle's, in 11 cells, k_rx's bcch +85 among them: guard symbols (0, 1 and the last three:
    nothing is sent there, no soft bit comes from them) whose noise sample, the mean taken out, was 160 ... 1070 times
    weaker than the burst's median.  The reference forms the mean as one serial fp32 sum over the window
    (osmo_cxvec_sig_normalize), which under an offset of the burst's amplitude ends 2e-7 ... 1.2e-6 from the float64 mean;
    the kernels' tree sums end within 1e-7 of it, and against a sample of 1e-3 that is 1e-4 ... 5e-4 of a soft-symbol
    step.  The soft symbols that k_rx and k_rx4g write out are now formed about the reference's own mean
    (window_mean_serial, rx_window.h), in calls that ask for them; soft bits and everything else are as before.  Largest
    distance since, over all cells: 3.1e-5 (it was 9.9e-5 in the cells that passed); freq_err: 1.2e-8."""
    c = cell_inputs(pkg, orc, cell)
    st = check_inputs(c)
    misses = []
    for kind in KINDS:
        big = _demod(gpu_api, c, c["shifts"][kind])
        res = _check(c, kind, big, misses=misses)
        print("demod4", cell_id(cell), d4.IMPL_NAME[cell[0]], kind, "safe share %.4f" % st["safe"], res)
        parts = [_demod(gpu_api, c, c["shifts"][kind], rows) for rows in _halves(c["n"])]
        print("demod4", cell_id(cell), kind, "against k_rx", _same_as_one_per_wave(c, kind, big, parts))
        if cell[0] == 0:
            # one step past the rule's limit the one call is k_rx's as well: the same answer to the bit
            for k in OUTPUTS:
                assert _same_bits(big[k], np.concatenate([p[k] for p in parts])), (cell, kind, k)
    # no shift array is an all-zero one, to the bit
    none = _demod(gpu_api, c, None)
    zero = _demod(gpu_api, c, np.zeros(c["n"], np.float32))
    for k in OUTPUTS:
        assert _same_bits(none[k], zero[k]), (cell, k)
    # (last, so that everything else about the cell is held whatever this finds)
    for m in misses:
        print("demod4 miss", m)
    assert not misses, ("%d soft symbols differ by 1e-4 or more" % len(misses), misses[:8])


# ---- edges ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cell", ONE_LAG, ids=cell_id)
def test_one_lag_window_has_no_power(gpu_api, orc, pkg, cell):
    """in_len == len * 4: one lag, where the reference's peak search finds no power (rv = -1) -- and nothing else comes out"""
    c = cell_inputs(pkg, orc, cell)
    assert c["n"] == 4097 and c["in_len"] == c["fmt"].length * 4
    for kind in KINDS:
        got = _demod(gpu_api, c, c["shifts"][kind])
        assert (c["ref"][kind].rv == -1).all() and (got["rv"] == -1).all(), (cell, kind, np.nonzero(got["rv"] != -1)[0][:8])
        for k in ("toa", "freq_err", "ebits", "ssyms"):
            assert not got[k].any() and not getattr(c["ref"][kind], k).any(), (cell, kind, k)


@gpu
@pytest.mark.parametrize("cell", STRIDED, ids=cell_id)
def test_strided_rows_and_absent_outputs(gpu_api, orc, pkg, cell):
    """The C entry itself: soft-bit rows 16 bytes further apart than they are long, in a buffer filled with 77, and no
    sync_id, freq_err or ssyms.  The rows, toa and rv are the plain call's, and the 16 bytes behind each row are still 77:
    k_rx4g and k_rx used to store zeros from a row's last soft bit up to its stride, and the host-pointer entry, which
    stages the buffer through the device, now sends it there first so that what the kernels leave alone comes back."""
    c = cell_inputs(pkg, orc, cell)
    fmt, n, fs = c["fmt"], c["n"], c["shifts"]["matching"]
    plain = _demod(gpu_api, c, fs)
    stride = fmt.ebits + 16
    eb = np.full((n, stride), 77, np.int8)
    toa, rv = np.full(n, 77, np.float32), np.full(n, 77, np.int32)
    rc = gpu_api._fn("gmr1_hip_demod_batch")(FORMATS.index(c["name"]), n, c["sps"], c["in_len"], c["iq"].ctypes.data, c["iq"].size,
                                             c["offset"].ctypes.data, fs.ctypes.data, eb.ctypes.data, stride, None, toa.ctypes.data,
                                             None, None, rv.ctypes.data)
    assert rc == 0
    assert np.array_equal(rv, plain["rv"]) and np.array_equal(toa.view(np.uint32), plain["toa"].view(np.uint32))
    assert np.array_equal(eb[:, :fmt.ebits], plain["ebits"])
    assert (eb[:, fmt.ebits:] == 77).all(), np.nonzero((eb[:, fmt.ebits:] != 77).any(axis=1))[0][:8]
    _check(c, "matching", dict(plain, ebits=np.ascontiguousarray(eb[:, :fmt.ebits]), toa=toa, rv=rv))
    # ... and of the first 2000 bursts alone, which take k_rx
    few = 2000
    small = _demod(gpu_api, c, fs, np.arange(few))
    eb[:] = 77
    rc = gpu_api._fn("gmr1_hip_demod_batch")(FORMATS.index(c["name"]), few, c["sps"], c["in_len"], c["iq"].ctypes.data, c["iq"].size,
                                             c["offset"].ctypes.data, fs.ctypes.data, eb.ctypes.data, stride, None, None, None,
                                             None, rv.ctypes.data)
    assert rc == 0
    assert np.array_equal(rv[:few], small["rv"]) and np.array_equal(eb[:few, :fmt.ebits], small["ebits"])
    assert (eb[:few, fmt.ebits:] == 77).all() and (eb[few:] == 77).all()


# ---- k_rx4g_tch3 ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cell", TCH3, ids=cell_id)
def test_tch3_rx_on_the_grid(gpu_api, orc, pkg, decoder, cell):
    """gmr1_hip_tch3_rx_batch on the NT3 speech cells: one launch (k_rx4g_tch3) up to +40; at +41 the rule leaves the small
    variant and the entry makes two launches.  Its demodulator is held to the oracle's by the module's rules; its frames,
    status bits and metrics are orc.tch3_decode's on the call's own soft bits, silent bursts included; every output is
    demod_batch's + tch3_decode_batch's to the bit; and leaving the soft bits out changes nothing else."""
    c = cell_inputs(pkg, orc, cell)
    n = c["n"]
    ciph = np.random.default_rng(cell[2]).integers(0, 2, (n, 208), dtype=np.uint8)
    for kind, m, cp in (("matching", 0, None), ("unrelated", 1, ciph), ("matching", 1, None), ("unrelated", 0, ciph)):
        fs = c["shifts"][kind]
        one = gpu_api.tch3_rx_batch(c["iq"], c["offset"], c["in_len"], sps=4, freq_shift=fs, m=m, ciph=cp)
        tag = (cell_id(cell), decoder, kind, "m", m, "ciphered" if cp is not None else "plain")
        print("tch3", tag, _check(c, kind, one, full=False))
        want = orc.tch3_decode(one["ebits"], m=m, ciph=cp)
        for k, w in zip(("frame0", "frame1", "bits_s", "conv0", "conv1"), want):
            assert np.array_equal(one[k], w), (tag, k, "against the oracle's decoder", np.nonzero(one[k].reshape(n, -1) != w.reshape(n, -1))[0][:8])
        d = _demod(gpu_api, c, fs)
        two = gpu_api.tch3_decode_batch(d["ebits"], m=m, ciph=cp)
        for k in ("rv", "sync_id", "toa", "ebits"):
            assert _same_bits(one[k], d[k]), (tag, k, "against demod_batch")
        for k, w in zip(("frame0", "frame1", "bits_s", "conv0", "conv1"), two):
            assert np.array_equal(one[k], w), (tag, k, "against tch3_decode_batch")
        lean = gpu_api.tch3_rx_batch(c["iq"], c["offset"], c["in_len"], sps=4, freq_shift=fs, m=m, ciph=cp, want_ebits=False)
        assert lean["ebits"] is None
        for k in ("rv", "sync_id", "toa", "frame0", "frame1", "bits_s", "conv0", "conv1"):
            assert _same_bits(lean[k], one[k]), (tag, k, "without the soft-bit output")
