"""The one-burst-per-wave demodulator (demod_one / k_rx, rx_one.h) against the oracle on every burst format at every
samples-per-symbol regime, with per-burst freq_shift, every burst compared.

launch_rx (rx_kernels.hip) picks k_rx<samples per lane, sps> by the window's length and sps; windows of len * sps + win
samples (win = 6 at sps 1, else 4 * sps) reach, by format (symbols per burst):

    sps  win   dc2 (78)  nt3_* (117)  bcch dc6 nt6 sdcch (234)  nt9 rach (351)  dc12 (468)
     1     6   <16, 0>   <16, 0>      <16, 0>                   <16, 0> *       <16, 0> *
     2     8   <16, 0>   <16, 0>      <16, 0>                   <16, 0> *       <16, 0> *
     3    12   <16, 0>   <16, 0>      <16, 0>                   <32, 0>         <32, 0>
     4    16   <16, 4>   <16, 4>      <16, 4>                   <32, 4>         <32, 4>
     5    20   <16, 0>   <16, 0>      <32, 0>                   <32, 0>         <64, 0>
     8    32   <16, 0>   <16, 0>      <32, 0>                   <64, 0>         <64, 0>
    11    44   <16, 0>   <32, 0>      <64, 0>                   <64, 0>         (5192 samples: refused)
    16    64   <32, 0>   <32, 0>      <64, 0>                   (refused)       (refused)
     4   100                          bcch: <32, 4> (1036 samples)
     4   200                                                                    <64, 0> (2072 samples, sps 4 at run time)

*: the six cells where a window of 1024 samples or fewer (16 samples per lane) holds a burst of more than 256 symbols: the
soft-symbol loop has to cover the burst's length, not what fits the smallest window.

Per cell 40 bursts (a random training sequence each where the format has several), a fraction of a sample and a few samples
of jitter, carrier offsets of 150 Hz rms, Es/N0 15 dB; demodulated with the shift that takes the offset out (what the receive
loop passes) and with an unrelated one.  Asserted on EVERY burst: rv == oracle's == 0, sync_id == oracle's, toa within
16 / 1024 of a sample.  Which bursts are compared in full -- freq_err to 1e-5, all `length` soft symbols
to 1e-4, all soft bits to 1 LSB -- is decided from the ORACLE's toa alone: a burst is safe when that toa is more than
32 / 1024 away from the nearest x.5 (the sample pick round(toa) cannot differ within the toa bound) and, below 4 samples
per symbol, | |toa - round(toa)| - 0.1 | > 32 / 1024 (neither can the choice of the fractional-delay branch,
pi4cxpsk.c:298).  At sps >= 4 every safe burst is compared; below, every safe burst whose toa is the oracle's to the bit
(the sinc delay is a function of toa), and the share of safe bursts where it is not is bounded over all sps < 4 cells."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

FORMATS = ["bcch", "dc2", "dc6", "dc12", "nt3_speech", "nt3_facch", "nt6", "nt9", "rach", "sdcch"]
LEN = dict(bcch=234, dc2=78, dc6=234, dc12=468, nt3_speech=117, nt3_facch=117, nt6=234, nt9=351, rach=351, sdcch=234)
SPS = [1, 2, 3, 4, 5, 8, 11, 16]
MAX_IN_LEN = 4096
N = 40
TOA_TOL = 16.0 / 1024.0
GUARD = 32.0 / 1024.0
KINDS = ("matching", "unrelated")


def _win(sps):
    return 6 if sps == 1 else 4 * sps


CELLS = [(sps, name, _win(sps)) for sps in SPS for name in FORMATS if LEN[name] * sps + _win(sps) <= MAX_IN_LEN]
CELLS += [(4, "dc12", 200), (4, "bcch", 100)]
MARKED = [(sps, name, _win(sps)) for sps in (1, 2) for name in ("dc12", "nt9", "rach")]
LOW = [c for c in CELLS if c[0] < 4]
# one cell per instantiation, for the reference's own call
PER_INSTANTIATION = {(16, 4): (4, "bcch", 16), (16, 0): (3, "dc6", 12), (32, 4): (4, "nt9", 16), (32, 0): (5, "sdcch", 20),
                     (64, 0): (8, "rach", 32)}


def _instantiation(in_len, sps):
    """k_rx<samples per lane, sps> as launch_rx picks it (the docstring's table)"""
    npl = 16 if in_len <= 1024 else 32 if in_len <= 2048 else 64
    return npl, 4 if sps == 4 and npl <= 32 else 0


def _id(cell):
    return "sps%d-%s-win%d" % cell


_cells = {}


def _cell(pkg, orc, cell, n=N, toa_jitter=None, esn0_db=15.0):
    """The cell's windows, its two shift arrays and the oracle's answers to both, computed once and left alone."""
    if cell in _cells:
        return _cells[cell]
    sps, name, win = cell
    fmt = pkg.api.burst_format(name)
    assert fmt.length == LEN[name]
    rng = np.random.default_rng(7000 + 1000 * FORMATS.index(name) + 16 * win + sps)
    bits = rng.integers(0, 2, size=(n, fmt.ebits), dtype=np.uint8)
    sid = rng.integers(0, len(fmt.sync), size=n)
    sym = pkg.synth.map_symbols(fmt, bits, sync_id=sid)
    jit = min(2 * sps, win // 4) if toa_jitter is None else toa_jitter
    bb = pkg.synth.synth_windows(fmt, sym, sps, win, rng, toa_jitter=jit, frac=sps >= 2, cfo_hz_std=150.0, esn0_db=esn0_db)
    assert bb.in_len == bb.stride == fmt.length * sps + win
    shifts = {"matching": (-bb.cfo * sps).astype(np.float32), "unrelated": rng.normal(0.0, 0.08, n).astype(np.float32)}
    c = dict(sps=sps, name=name, win=win, fmt=fmt, dpos=fmt.data_positions(), bits=bits, iq=bb.iq, in_len=bb.in_len,
             offset=(np.arange(n) * bb.stride).astype(np.uint64), shifts=shifts, ref={}, safe={})
    for kind, fs in shifts.items():
        ref = [orc.demod(name, bb.iq[i], sps, float(fs[i])) for i in range(n)]
        toa = np.array([o["toa"] for o in ref], np.float64)
        off = np.abs(toa - np.floor(toa + 0.5))                   # |toa - round(toa)|, C's roundf on a toa >= 0
        safe = np.abs(off - 0.5) > GUARD
        if sps < 4:
            safe &= np.abs(off - 0.1) > GUARD
        c["ref"][kind], c["safe"][kind] = ref, safe
    _cells[cell] = c
    return c


def _compare_full(c, got, i, o, tag, misses):
    """freq_err, every soft symbol and every soft bit of burst i -> the number of midpoint exceptions among the soft bits;
    soft symbols beyond the tolerance are appended to `misses` (the cell's whole list is worth more than its first entry)"""
    fmt = c["fmt"]
    assert abs(float(got["freq_err"][i]) - o["freq_err"]) < 1e-5, (tag, "freq_err", got["freq_err"][i], o["freq_err"])
    assert got["ssyms"][i].shape == o["ssyms"].shape == (fmt.length,)
    d = np.abs(got["ssyms"][i].astype(np.float64) - o["ssyms"])
    d = np.minimum(d, np.abs(d - 2.0 ** fmt.nbits))               # on the circle of 2 ** nbits
    for k in np.nonzero(~(d < 1e-4))[0]:
        misses.append((tag, "symbol", int(k), "gpu", float(got["ssyms"][i][k]), "oracle", float(o["ssyms"][k])))
    return _compare_ebits(c, got["ebits"][i], o, tag)


def _compare_ebits(c, ebits, o, tag):
    """soft bits within 1 LSB, but for a symbol whose phase sits on the midpoint between two constellation points within the
    soft-symbol tolerance (identified through the oracle's soft symbol, as test_gpu_rx._compare_fused does): nearest point
    and neighbour swap roles, which flips the weakest possible soft bit, |value| = 63, and nothing else -> their number"""
    fmt = c["fmt"]
    assert ebits.shape == o["ebits"].shape == (fmt.ebits,)
    deb = np.abs(ebits.astype(int) - o["ebits"].astype(int))
    n_mid = 0
    for e in np.nonzero(deb > 1)[0]:
        sym = int(c["dpos"][e // fmt.nbits])
        what = (tag, "soft bit", int(e), "of symbol", sym, int(ebits[e]), int(o["ebits"][e]), float(o["ssyms"][sym]))
        assert abs(abs(float(o["ssyms"][sym])) % 1.0 - 0.5) < 1e-4, what
        assert abs(abs(int(ebits[e])) - 63) <= 1 and abs(abs(int(o["ebits"][e])) - 63) <= 1, what
        n_mid += 1
    return n_mid


def _enough_safe(c, kind):
    safe = c["safe"][kind]
    assert safe.size == N and safe.sum() >= 20, (c["sps"], c["name"], kind, "only %d of %d bursts are safe" % (safe.sum(), safe.size))


def _check(c, kind, got, need_safe=True):
    """got (demod_batch's answer to c's windows with the shifts of `kind`) against the oracle, by the module's rules ->
    dict(safe, differ: safe bursts whose toa is not the oracle's to the bit, compared, on / off: compared bursts on either
    side of the fractional-delay branch)"""
    sps, fmt, ref, safe = c["sps"], c["fmt"], c["ref"][kind], c["safe"][kind]
    n = len(ref)
    if need_safe:
        _enough_safe(c, kind)
    st = dict(safe=int(safe.sum()), differ=0, compared=0, on=0, off=0)
    n_mid, misses = 0, []
    for i in range(n):
        o = ref[i]
        tag = (sps, c["name"], c["win"], kind, "burst", i)
        assert got["rv"][i] == o["rv"] == 0, (tag, "rv", got["rv"][i], o["rv"])
        assert got["sync_id"][i] == o["sync_id"], (tag, "sync_id", got["sync_id"][i], o["sync_id"])
        assert abs(float(got["toa"][i]) - o["toa"]) < TOA_TOL, (tag, "toa", got["toa"][i], o["toa"])
        if not safe[i]:
            continue
        if sps < 4 and float(got["toa"][i]) != o["toa"]:
            st["differ"] += 1
            continue
        n_mid += _compare_full(c, got, i, o, tag, misses)
        st["compared"] += 1
        frac_on = sps < 4 and abs(o["toa"] - np.floor(o["toa"] + 0.5)) > 0.1
        st["on" if frac_on else "off"] += 1
    assert not misses, ("%d soft symbols differ by 1e-4 or more" % len(misses), misses[:8])
    bits = st["compared"] * fmt.ebits
    assert n_mid <= max(1, int(2e-5 * bits)), (sps, c["name"], kind, "%d midpoint symbols in %d soft bits" % (n_mid, bits))
    return st


def _sent_bits_come_back(c):
    """input sanity, on the oracle's side: with the matching shift the oracle's hard decisions are the sent bits (single
    training sequence only: with several the reference's correlation accumulator, never cleared between them, picks
    the wrong one about half the time -- GPU == oracle is the contract there)"""
    if len(c["fmt"].sync) != 1:
        return
    hard = np.array([(o["ebits"] < 0) for o in c["ref"]["matching"]], np.uint8)
    ber = (hard != c["bits"]).mean()
    assert ber <= 0.02, (c["sps"], c["name"], "the oracle gets %.4f of the sent bits wrong" % ber)


_got = {}


def _gpu(gpu_api, c, kind):
    """demod_batch's answer to the cell's windows with the shifts of `kind`, asked for once"""
    key = (c["sps"], c["name"], c["win"], kind)
    if key not in _got:
        _got[key] = gpu_api.demod_batch(c["name"], c["iq"], c["offset"], c["in_len"], sps=c["sps"], freq_shift=c["shifts"][kind])
    return _got[key]


def test_grid_reaches_every_instantiation():
    reached = {_instantiation(LEN[name] * sps + win, sps) for sps, name, win in CELLS}
    assert reached == {(16, 4), (16, 0), (32, 4), (32, 0), (64, 0)}
    assert len(CELLS) == 78 and len(LOW) == 30
    for cell in MARKED:
        assert cell in CELLS and _instantiation(LEN[cell[1]] * cell[0] + cell[2], cell[0]) == (16, 0) and LEN[cell[1]] > 256
    assert _instantiation(LEN["dc12"] * 4 + 200, 4) == (64, 0) and _instantiation(LEN["bcch"] * 4 + 100, 4) == (32, 4)
    for inst, (sps, name, win) in PER_INSTANTIATION.items():
        assert (sps, name, win) in CELLS and _instantiation(LEN[name] * sps + win, sps) == inst


def test_grid_inputs_on_the_oracle(orc, pkg):
    """What the GPU tests below rest on holds with the oracle alone: every cell has its 20 safe bursts under either shift,
    and the oracle gives back the sent bits where it can"""
    worst = min((int(_cell(pkg, orc, cell)["safe"][kind].sum()), _id(cell), kind) for cell in CELLS for kind in KINDS)
    print("fewest safe bursts:", worst)
    for cell in CELLS:
        c = _cell(pkg, orc, cell)
        for kind in KINDS:
            _enough_safe(c, kind)
        _sent_bits_come_back(c)


@gpu
@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_demod_grid(gpu_api, orc, pkg, cell):
    """Two things this grid found are held by it.  The six starred cells: soft symbols and soft bits from symbol 256 on were
    never computed in a window of 1024 samples or fewer.  sps1-nt9-win6 (bursts 21 and 24, symbols 348 and 335) and
    sps3-dc12-win12 (burst 35, symbol 465), matching shift: a sample 15 ... 60 times weaker than the burst's median behind the
    sinc fractional delay, where the reference's fp32 rounding of the per-sample derotation fs * n (3e-5 rad at 730 rad) is
    1.2 ... 1.4e-4 of a soft-symbol step and has to be the kernel's too (delayed_sample, rx_one.h)."""
    c = _cell(pkg, orc, cell)
    _sent_bits_come_back(c)
    for kind in KINDS:
        print(_id(cell), kind, _check(c, kind, _gpu(gpu_api, c, kind)))
    # no shift array is an all-zero one, to the bit
    none = gpu_api.demod_batch(c["name"], c["iq"], c["offset"], c["in_len"], sps=c["sps"], freq_shift=None)
    zero = gpu_api.demod_batch(c["name"], c["iq"], c["offset"], c["in_len"], sps=c["sps"], freq_shift=np.zeros(N, np.float32))
    for k in none:
        assert np.array_equal(none[k].view(np.uint8), zero[k].view(np.uint8)), (cell, k)
    assert not none["rv"].any()


@gpu
def test_toa_parity_below_four_samples_per_symbol(gpu_api, orc, pkg):
    """Below 4 samples per symbol a toa one bisection step off the oracle's legitimately moves the sinc delay, so those bursts
    are not compared in full: they have to be rare.  The bound is test_gpu_rx._compare_fused's `near` bound, DESIGN.md
    section 6's measured 0 ... 0.25 % doubled; what this measures stands in DESIGN.md section 6."""
    tot = dict(safe=0, differ=0, on=0, off=0)
    for cell in LOW:
        c = _cell(pkg, orc, cell)
        for kind in KINDS:
            got, safe = _gpu(gpu_api, c, kind), c["safe"][kind]
            toa = np.array([o["toa"] for o in c["ref"][kind]], np.float32)
            assert np.abs(got["toa"].astype(np.float64) - toa).max() < TOA_TOL, (cell, kind)
            same = got["toa"] == toa
            on = np.abs(toa - np.floor(toa + np.float32(0.5))) > 0.1
            tot["safe"] += int(safe.sum())
            tot["differ"] += int((safe & ~same).sum())
            tot["on"] += int((safe & same & on).sum())
            tot["off"] += int((safe & same & ~on).sum())
    print("sps < 4: %(differ)d of %(safe)d safe bursts have a toa that is not the oracle's; of the others %(on)d went through "
          "the fractional delay and %(off)d did not" % tot)
    assert tot["safe"] >= 20 * 2 * len(LOW)
    assert tot["differ"] <= 0.005 * tot["safe"], tot
    # both sides of the fractional-delay branch (pi4cxpsk.c:298) are among the bursts compared in full
    assert tot["on"] >= 200 and tot["off"] >= 200, tot


# ---- edges ---------------------------------------------------------------------------------------------------------------
EDGE_CELLS = [(4, "rach"), (2, "nt9"), (1, "dc12"), (8, "nt3_facch")]


@gpu
@pytest.mark.parametrize("sps,name", EDGE_CELLS)
def test_one_lag_window_has_no_power(gpu_api, orc, pkg, sps, name):
    """in_len == len * sps: one lag, where the reference's peak search finds no power (rv = -1) -- and nothing else comes out"""
    c = _cell(pkg, orc, (sps, name, 0), n=8, toa_jitter=0)
    for kind in KINDS:
        got = gpu_api.demod_batch(name, c["iq"], c["offset"], c["in_len"], sps=sps, freq_shift=c["shifts"][kind])
        for i, o in enumerate(c["ref"][kind]):
            assert got["rv"][i] == o["rv"] == -1, (sps, name, kind, i, got["rv"][i], o["rv"])
        for k in ("toa", "freq_err", "ebits", "ssyms"):
            assert not got[k].any(), (sps, name, kind, k)


@gpu
@pytest.mark.parametrize("sps,name", EDGE_CELLS)
def test_two_lag_window(gpu_api, orc, pkg, sps, name):
    """in_len == len * sps + 1: two lags, the smallest window that demodulates (the burst is not aligned to either, so what
    comes out is compared, not looked at)"""
    c = _cell(pkg, orc, (sps, name, 1), n=8, toa_jitter=0)
    for kind in KINDS:
        got = gpu_api.demod_batch(name, c["iq"], c["offset"], c["in_len"], sps=sps, freq_shift=c["shifts"][kind])
        print(sps, name, kind, _check(c, kind, got, need_safe=False))


@gpu
@pytest.mark.parametrize("sps,name", [(11, "dc12"), (16, "nt9")])
def test_window_beyond_4096_samples_is_refused(gpu_api, pkg, sps, name):
    fmt = pkg.api.burst_format(name)
    n, in_len = 2, fmt.length * sps + _win(sps)
    assert in_len > MAX_IN_LEN
    iq = np.zeros(n * in_len, np.complex64)
    offset = (np.arange(n) * in_len).astype(np.uint64)
    with pytest.raises(gpu_api.Gmr1HipError):
        gpu_api.demod_batch(name, iq, offset, in_len, sps=sps)
    # ... and the caller's outputs are left as they were
    out = [np.full((n, fmt.ebits), 77, np.int8), np.full(n, 77, np.int32), np.full(n, 77, np.float32),
           np.full(n, 77, np.float32), np.full((n, fmt.length), 77, np.float32), np.full(n, 77, np.int32)]
    eb, sid, toa, fe, ss, rv = [a.ctypes.data for a in out]
    rc = gpu_api._fn("gmr1_hip_demod_batch")(FORMATS.index(name), n, sps, in_len, iq.ctypes.data, iq.size, offset.ctypes.data,
                                             None, eb, fmt.ebits, sid, toa, fe, ss, rv)
    assert rc != 0
    for a in out:
        assert (a == 77).all()


# ---- the reference's own call, and the debugging entry -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cell", list(PER_INSTANTIATION.values()) + MARKED, ids=_id)
def test_reference_call_on_the_grid(gpu_api, orc, pkg, cell):
    """gmr1_pi4cxpsk_demod on burst 0 of the cell (and on its first safe burst, should burst 0 not be one) by the same rules"""
    c = _cell(pkg, orc, cell)
    sps, fs, safe, ref = c["sps"], c["shifts"]["matching"], c["safe"]["matching"], c["ref"]["matching"]
    for i in sorted({0, int(np.argmax(safe))}):
        g = gpu_api.pi4cxpsk_demod(c["name"], c["iq"][i], sps, float(fs[i]))
        o = ref[i]
        tag = (cell, "burst", i)
        assert g["rv"] == o["rv"] == 0, tag
        assert g["sync_id"] == o["sync_id"], tag
        assert abs(g["toa"] - o["toa"]) < TOA_TOL, (tag, g["toa"], o["toa"])
        if safe[i] and (sps >= 4 or g["toa"] == o["toa"]):
            assert abs(g["freq_err"] - o["freq_err"]) < 1e-5, tag
            assert _compare_ebits(c, g["ebits"], o, tag) <= 1


@gpu
@pytest.mark.parametrize("cell", [(2, "nt9", 8), (1, "dc12", 6)], ids=_id)
def test_demod_taps_on_a_long_burst_in_a_small_window(gpu_api, orc, pkg, cell):
    """gmr1_hip_demod_taps shares demod_one: its ordinary outputs are the batch entry's, over the whole burst"""
    c = _cell(pkg, orc, cell)
    fs = c["shifts"]["matching"]
    got = gpu_api.demod_batch(c["name"], c["iq"], c["offset"], c["in_len"], sps=c["sps"], freq_shift=fs)
    for i in (0, int(np.argmax(c["safe"]["matching"]))):
        t = gpu_api.demod_taps(c["name"], c["iq"][i], sps=c["sps"], freq_shift=float(fs[i]))
        assert t["rv"] == got["rv"][i] == 0
        assert t["toa"] == got["toa"][i] and t["freq_err"] == got["freq_err"][i] and t["sync_id"] == got["sync_id"][i]
        assert np.array_equal(t["ssyms"], got["ssyms"][i]) and np.array_equal(t["ebits"], got["ebits"][i]), (cell, i)
