"""The shaped modulator (k_shape, tx_kernels.hip; gmr1_hip_shape_batch*, gmr1_hip_mod_shaped_batch*) on the GPU.

1. Every sample against a float64 restatement of the arithmetic (symbols from mod_batch with the burst's own training
   sequence, pulses from synth.rc_pulse / rrc_pulse), under a DERIVED bound per sample:
       2^-23 gain [ (2 span + 4) sum_m |g_m| + (2 |phase| + 4) |body64| ]
   first term: the coefficients' rounding and 2 span + 1 accumulations in any order, fused or not; second: two roundings of
   the phase, sincosf, the complex product and the gain.  Outside the body the bound is 0: those samples are zeros.
2. Exact: bits in one launch = shape_batch on mod_batch's symbols; a burst's window does not depend on its batch; NULL
   impairments = 0 / 0 / 0 / 0 / 1; nothing outside the windows is written and everything inside is; _dev = host form.
3. Through the demodulator, noise-free: every bit, and the arrival time it reports on these windows is the one it reports
   on the restatement's.
4. The closed loop encode -> mod_shaped -> demod -> decode for RACH and DC12."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

FORMATS = ["bcch", "dc2", "dc6", "dc12", "nt3_speech", "nt3_facch", "nt6", "nt9", "rach", "sdcch"]
LEN = dict(bcch=234, dc2=78, dc6=234, dc12=468, nt3_speech=117, nt3_facch=117, nt6=234, nt9=351, rach=351, sdcch=234)
SPS = (1, 2, 3, 4, 5, 8, 16)
SYM_RATE = 23400
MAX_IN_LEN = 4096
TOA_TOL = 16.0 / 1024.0


def _win(sps):
    return 6 if sps == 1 else 4 * sps


# (format, sps, pulse, span)
CELLS = [(name, 4, "rc", 5) for name in FORMATS]
CELLS += [(name, sps, pulse, 5) for name in ("bcch", "nt3_facch", "dc12") for sps in SPS for pulse in ("rc", "rrc")
          if (name, sps, pulse, 5) not in CELLS]
CELLS += [("dc2", sps, "rc", span) for sps in (3, 16) for span in (1, 3, 8)]


def _id(cell):
    return "%s-sps%d-%s-span%d" % cell


def _symbols(api, name, bits, sid):
    """mod_batch with each burst's own training sequence"""
    sym = np.zeros((bits.shape[0], LEN[name]), np.complex64)
    for s in np.unique(sid):
        rows = np.nonzero(sid == s)[0]
        sym[rows] = api.mod_batch(name, bits[rows], int(s))
    return sym


def _impairments(rng, n, sps, in_len, win, jitter, clip=True):
    """The per-burst arrays of a cell: n bursts around win / 2, and with `clip` two more that leave the window on either side"""
    start = win // 2 + rng.integers(-jitter, jitter + 1, n)
    if clip:
        start = np.concatenate([start, [-3 * sps, in_len - 2 * sps]])
    m = start.size
    frac = rng.uniform(-0.5, 0.5, m) if sps > 1 else np.zeros(m)
    cfo = rng.normal(0.0, 150.0, m) * (2 * np.pi / (SYM_RATE * sps))
    return dict(start=start.astype(np.int32), frac=frac.astype(np.float32), cfo=cfo.astype(np.float32),
                phase0=rng.uniform(0, 2 * np.pi, m).astype(np.float32),
                gain=(10.0 ** (rng.normal(0.0, 3.0, m) / 20.0)).astype(np.float32))


def restate(synth, sym, sps, in_len, pulse, span, start=None, frac=None, cfo=None, phase0=None, gain=None):
    """The header's formula in float64 -> (windows complex128 (n, in_len), the bound per sample)"""
    n, L = sym.shape
    g = synth.rrc_pulse if pulse == "rrc" else synth.rc_pulse
    f64 = lambda a, d: np.full(n, d, np.float64) if a is None else np.asarray(a).astype(np.float64)
    start, frac, cfo, phase0, gain = f64(start, 0).astype(np.int64), f64(frac, 0), f64(cfo, 0), f64(phase0, 0), f64(gain, 1)
    k = np.arange(in_len, dtype=np.int64)
    mi = np.arange(2 * span + 1)
    x = np.zeros((n, in_len), np.complex128)
    bound = np.zeros((n, in_len))
    for b in range(n):
        q = k - (start[b] - span * sps)
        ok = (q >= 0) & (q < (L + 2 * span) * sps)
        if not ok.any():
            continue
        i, p = q[ok] // sps, q[ok] % sps
        spad = np.zeros(L + 4 * span, np.complex128)
        spad[2 * span:2 * span + L] = sym[b]
        G = g((mi - span)[:, None] + (np.arange(sps)[None, :] - frac[b]) / sps)           # (taps, sps)
        body = (spad[i[None, :] + 2 * span - mi[:, None]] * G[:, p]).sum(0)
        ph = phase0[b] + cfo[b] * k[ok]
        x[b, ok] = gain[b] * np.exp(1j * ph) * body
        bound[b, ok] = 2.0 ** -23 * gain[b] * ((2 * span + 4) * np.abs(G[:, p]).sum(0) + (2 * np.abs(ph) + 4) * np.abs(body))
    return x, bound


_cells = {}


def _cell(api, synth, cell):
    """The cell's inputs, the kernel's windows and the restatement, computed once and left alone"""
    if cell in _cells:
        return _cells[cell]
    name, sps, pulse, span = cell
    rng = np.random.default_rng(9000 + 100 * FORMATS.index(name) + 7 * sps + span + (pulse == "rrc"))
    info = api.burst_info(name)
    win = _win(sps)
    in_len = LEN[name] * sps + win
    imp = _impairments(rng, 8, sps, in_len, win, min(2 * sps, max(win // 4, 1)))
    n = imp["start"].size
    bits = rng.integers(0, 2, (n, info.ebits), dtype=np.uint8)
    sid = rng.integers(0, info.n_sync, n).astype(np.int32)
    sym = _symbols(api, name, bits, sid)
    got = api.mod_shaped_batch(name, bits, sps, in_len, sync_id=sid, pulse=pulse, span=span, **imp)
    want, bound = restate(synth, sym, sps, in_len, pulse, span, **imp)
    c = dict(name=name, sps=sps, pulse=pulse, span=span, in_len=in_len, win=win, bits=bits, sid=sid, sym=sym, imp=imp, got=got,
             want=want, bound=bound)
    _cells[cell] = c
    return c


_worst = {}


@gpu
@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_every_sample_within_the_derived_bound(gpu_api, pkg, cell):
    c = _cell(gpu_api, pkg.synth, cell)
    got, want, bound = c["got"], c["want"], c["bound"]
    assert got.shape == want.shape == (10, c["in_len"]) and got.dtype == np.complex64
    err = np.abs(got.astype(np.complex128) - want)
    inside = bound > 0
    ratio = (err[inside] / bound[inside]).max()
    _worst[cell] = ratio
    print("%s: worst error / bound %.3f over %d samples (overall so far %.3f)" % (_id(cell), ratio, inside.sum(), max(_worst.values())))
    # the two clipped bursts: the body leaves the window on the left / on the right, and part of a window stays empty
    assert inside[8, 0] and not inside[9, 0] and inside[9, -1] and c["imp"]["start"][8] < 0
    assert inside[:8].any(1).all()
    assert not got[~inside].any(), "a sample outside the body is not zero"
    assert (err <= bound).all(), (ratio, np.argwhere(err > bound)[:5])


@gpu
@pytest.mark.parametrize("cell", [("nt3_facch", 4, "rc", 5), ("nt3_facch", 1, "rc", 5), ("dc12", 3, "rrc", 5), ("nt6", 4, "rc", 5),
                                  ("dc2", 16, "rc", 8)], ids=_id)
def test_bits_in_one_launch_equal_shaping_the_modulators_symbols(gpu_api, pkg, cell):
    c = _cell(gpu_api, pkg.synth, cell)
    two = gpu_api.shape_batch(c["sym"], c["sps"], c["in_len"], pulse=c["pulse"], span=c["span"], **c["imp"])
    assert two.tobytes() == c["got"].tobytes()
    if gpu_api.burst_info(c["name"]).n_sync > 1:
        assert len(set(c["sid"].tolist())) > 1


@gpu
@pytest.mark.parametrize("length,sps,span", [(2006, 2, 5), (2007, 2, 5), (2048, 16, 8), (1, 3, 1)],
                         ids=["four-waves-a-block", "three-waves-a-block", "longest-body", "one-symbol"])
def test_symbol_rows_up_to_the_longest(gpu_api, pkg, length, sps, span):
    """Symbols from memory at the lengths where the launch changes shape: a work-group holds four bursts while their symbols
    fit 64 KiB of LDS (len 2006 at span 5, sps 2) and three from there on; len 2048 at span 8, sps 16 is the longest body."""
    rng = np.random.default_rng(length)
    n, win = 7, 4 * sps
    in_len = length * sps + win
    sym = np.exp(1j * rng.uniform(0, 2 * np.pi, (n, length))).astype(np.complex64)
    imp = _impairments(rng, n - 2, sps, in_len, win, sps)
    got = gpu_api.shape_batch(sym, sps, in_len, pulse="rrc", span=span, **imp)
    want, bound = restate(pkg.synth, sym, sps, in_len, "rrc", span, **imp)
    err = np.abs(got.astype(np.complex128) - want)
    inside = bound > 0
    print("len %d: worst error / bound %.3f" % (length, (err[inside] / bound[inside]).max()))
    assert inside[:n - 2].any(1).all() and not got[~inside].any()
    assert (err <= bound).all()


def _batch67(api):
    rng = np.random.default_rng(67)
    n, name, sps = 67, "nt3_speech", 4
    in_len = LEN[name] * sps + 16
    imp = _impairments(rng, n, sps, in_len, 16, 4, clip=False)
    bits = rng.integers(0, 2, (n, api.burst_info(name).ebits), dtype=np.uint8)
    return name, sps, in_len, imp, bits


@gpu
def test_a_window_does_not_depend_on_its_batch(gpu_api):
    name, sps, in_len, imp, bits = _batch67(gpu_api)
    cut = lambda rows: {k: v[rows] for k, v in imp.items()}
    full = gpu_api.mod_shaped_batch(name, bits, sps, in_len, **imp)
    assert full.shape == (67, in_len)
    for n in (3, 5):
        part = gpu_api.mod_shaped_batch(name, bits[:n], sps, in_len, **cut(slice(0, n)))
        assert part.tobytes() == full[:n].tobytes(), n
    for i in (0, 1, 2, 3, 4, 63, 64, 66):
        alone = gpu_api.mod_shaped_batch(name, bits[i:i + 1], sps, in_len, **cut(slice(i, i + 1)))
        assert alone.tobytes() == full[i:i + 1].tobytes(), i


@gpu
def test_left_out_impairments_are_0_0_0_0_1(gpu_api):
    name, sps, in_len, imp, bits = _batch67(gpu_api)
    bits = bits[:5]
    z, one = np.zeros(5, np.float32), np.ones(5, np.float32)
    none = gpu_api.mod_shaped_batch(name, bits, sps, in_len)
    given = gpu_api.mod_shaped_batch(name, bits, sps, in_len, start=np.zeros(5, np.int32), frac=z, cfo=z, phase0=z, gain=one)
    assert none.tobytes() == given.tobytes() and none.any(1).all()
    sym = gpu_api.mod_batch(name, bits, 0)
    a = gpu_api.shape_batch(sym, sps, in_len)
    b = gpu_api.shape_batch(sym, sps, in_len, start=0, frac=0.0, cfo=0.0, phase0=0.0, gain=1.0)
    assert a.tobytes() == b.tobytes() == none.tobytes()
    # symbol 0 lands on sample `start`: at frac 0 the raised cosine has no intersymbol interference
    at = gpu_api.shape_batch(sym, sps, in_len, start=8)
    assert np.abs(at[:, 8:8 + LEN[name] * sps:sps] - sym).max() < 1e-6


SENT = np.float32(-7.25)


def _gapped(n, in_len):
    """windows with gaps of 1, 2, 3, ... samples between them and in front: every other one starts on an odd sample"""
    off = np.cumsum(np.arange(1, n + 1) % 4 + in_len) - in_len
    return off.astype(np.uint64), int(off[-1]) + in_len + 5


@gpu
@pytest.mark.parametrize("sps,in_len", [(4, 484), (4, 483), (1, 41), (16, 700)])
def test_nothing_outside_the_windows_is_written_and_dev_equals_host(gpu_api, pkg, sps, in_len):
    import torch
    api = gpu_api
    name, n, span = "nt3_speech", 7, 5
    rng = np.random.default_rng(in_len)
    imp = _impairments(rng, n - 2, sps, in_len, 16, 3)
    bits = rng.integers(0, 2, (n, api.burst_info(name).ebits), dtype=np.uint8)
    off, out_len = _gapped(n, in_len)
    inside = np.zeros(out_len, bool)
    for o in off:
        inside[int(o):int(o) + in_len] = True
    assert (~inside).sum() >= n and len(set((off % 2).tolist())) == 2
    # host form
    out = np.full(2 * out_len, SENT, np.float32).view(np.complex64)
    ret = api.mod_shaped_batch(name, bits, sps, in_len, offset=off, out=out, **imp)
    assert ret is out
    assert (out[~inside].view(np.float32) == SENT).all()
    assert not (out[inside].view(np.float32) == SENT).any()
    want, bound = restate(pkg.synth, api.mod_batch(name, bits, 0), sps, in_len, "rc", span, **imp)
    win = np.stack([out[int(o):int(o) + in_len] for o in off])
    assert not win[bound == 0].any() and (bound == 0).any()
    assert (np.abs(win - want) <= bound).all()
    dense = api.mod_shaped_batch(name, bits, sps, in_len, **imp)
    assert win.tobytes() == dense.tobytes()                     # ... wherever the windows lie
    # device form: the kernel itself leaves the gaps alone
    dev = lambda a: torch.from_numpy(a).cuda()
    t_out = torch.full((2 * out_len,), float(SENT), dtype=torch.float32, device="cuda")
    t = dict(bits=dev(bits), off=dev(off.view(np.int64)), **{k: dev(v) for k, v in imp.items()})
    st = torch.cuda.current_stream().cuda_stream
    api.mod_shaped_batch_dev(st, name, n, sps, api.PULSE_RC, span, in_len, t["bits"].data_ptr(), None, t["off"].data_ptr(),
                             t["start"].data_ptr(), t["frac"].data_ptr(), t["cfo"].data_ptr(), t["phase0"].data_ptr(),
                             t["gain"].data_ptr(), t_out.data_ptr(), out_len)
    torch.cuda.synchronize()
    assert t_out.cpu().numpy().tobytes() == out.tobytes()
    # symbols from memory, device form
    sym = api.mod_batch(name, bits, 0)
    t_sym = dev(sym.view(np.float32))
    t_out2 = torch.full((2 * out_len,), float(SENT), dtype=torch.float32, device="cuda")
    api.shape_batch_dev(st, n, LEN[name], sps, api.PULSE_RC, span, in_len, t_sym.data_ptr(), t["off"].data_ptr(),
                        t["start"].data_ptr(), t["frac"].data_ptr(), t["cfo"].data_ptr(), t["phase0"].data_ptr(),
                        t["gain"].data_ptr(), t_out2.data_ptr(), out_len)
    torch.cuda.synchronize()
    assert t_out2.cpu().numpy().tobytes() == out.tobytes()


@gpu
def test_no_bursts_and_bad_arguments_touch_nothing(gpu_api):
    api = gpu_api
    out = np.full(64, SENT, np.float32).view(np.complex64)
    keep = out.tobytes()
    f = api._fn("gmr1_hip_shape_batch")
    m = api._fn("gmr1_hip_mod_shaped_batch")
    sym = np.ones(8, np.complex64)
    off = np.zeros(1, np.uint64)
    p = lambda a: a.ctypes.data
    assert f(0, 8, 4, 0, 5, 32, None, None, None, None, None, None, None, None, 0) == 0
    assert m(0, 0, 4, 0, 5, 32, None, None, None, None, None, None, None, None, None, 0) == 0
    assert f(1, 8, 4, 0, 5, 32, p(sym), p(off), None, None, None, None, None, p(out), 31) == -22      # leaves out
    assert f(1, 8, 17, 0, 5, 32, p(sym), p(off), None, None, None, None, None, p(out), 32) == -22
    assert f(1, 8, 4, 0, 9, 32, p(sym), p(off), None, None, None, None, None, p(out), 32) == -22
    assert f(1, 8, 4, 3, 5, 32, p(sym), p(off), None, None, None, None, None, p(out), 32) == -22
    assert out.tobytes() == keep
    assert f(1, 8, 4, 0, 5, 32, p(sym), p(off), None, None, None, None, None, p(out), 32) == 0
    assert out.any() and out.tobytes() != keep


# ---- through the demodulator ----
DEMOD_CELLS = [(name, sps) for name in ("bcch", "dc2", "dc6", "dc12", "nt3_speech", "rach") for sps in (2, 3, 4, 5, 8, 16)
               if LEN[name] * sps + _win(sps) <= MAX_IN_LEN]


@gpu
@pytest.mark.parametrize("name,sps", DEMOD_CELLS, ids=lambda v: str(v))
def test_the_demodulator_reads_the_windows(gpu_api, pkg, name, sps):
    api = gpu_api
    n, span, win = 12, 5, _win(sps)
    in_len = LEN[name] * sps + win
    rng = np.random.default_rng(500 + 20 * FORMATS.index(name) + sps)
    imp = _impairments(rng, n, sps, in_len, win, min(2 * sps, win // 4), clip=False)
    del imp["gain"]
    bits = rng.integers(0, 2, (n, api.burst_info(name).ebits), dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * np.uint64(in_len)
    iq = api.mod_shaped_batch(name, bits, sps, in_len, **imp)
    shift = (-imp["cfo"].astype(np.float64) * sps).astype(np.float32)
    d = api.demod_batch(name, iq, off, in_len, sps=sps, freq_shift=shift, want_ssyms=False)
    assert not d["rv"].any()
    assert np.array_equal(d["ebits"] < 0, bits.astype(bool))
    want, _ = restate(pkg.synth, api.mod_batch(name, bits, 0), sps, in_len, "rc", span, **imp)
    r = api.demod_batch(name, want.astype(np.complex64), off, in_len, sps=sps, freq_shift=shift, want_ssyms=False)
    assert not r["rv"].any()
    print("%s sps %d: toa differs by at most %.5f" % (name, sps, np.abs(d["toa"] - r["toa"]).max()))
    assert (np.abs(d["toa"].astype(np.float64) - r["toa"]) <= TOA_TOL).all()


# ---- the closed loop ----
@gpu
@pytest.mark.parametrize("chain,burst", [("rach", "rach"), ("xch_dc12", "dc12")])
def test_closed_loop_payloads_come_back(gpu_api, chain, burst):
    api = gpu_api
    n, sps, win = 64, 4, 16
    rng = np.random.default_rng(41)
    if chain == "rach":
        pay = rng.integers(0, 256, (n, 18), dtype=np.uint8)
        pay[:, 17] &= 0x07
        sb = rng.integers(0, 256, n, dtype=np.uint8)
        eb = api.rach_encode_batch(pay, sb)
    else:
        pay = rng.integers(0, 256, (n, 24), dtype=np.uint8)
        eb = api.xch_dc12_encode_batch(pay)
    in_len = LEN[burst] * sps + win
    iq = api.mod_shaped_batch(burst, eb, sps, in_len, start=win // 2)
    d = api.demod_batch(burst, iq, np.arange(n, dtype=np.uint64) * np.uint64(in_len), in_len, sps=sps, want_ssyms=False)
    assert not d["rv"].any()
    assert np.array_equal(d["ebits"] < 0, eb.astype(bool))
    if chain == "rach":
        dec, rv, _, _ = api.rach_decode_batch(d["ebits"], sb)
        assert not rv.any() and np.array_equal(dec, pay)
    else:
        l2, crc, _ = api.xch_dc12_decode_batch(d["ebits"])
        assert not crc.any() and np.array_equal(l2, pay)
