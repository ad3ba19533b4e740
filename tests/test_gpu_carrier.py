"""The carrier mixer (k_carrier_mix, carrier_kernels.hip; gmr1_hip_carrier_mix*) and the FCCH chirp windows (k_chirp,
tx_kernels.hip; gmr1_hip_fcch_chirp_batch*) on the GPU.

1. Overlap-add, exact (sigma = 0, cfo = 0): bit for bit a float32 numpy loop in list order (carrier_ref.overlap_add_f32).
2. Rotation: every sample against the float64 rotation of the exact sums, under the roundings of step 2 counted in units of
   2^-23 |acc| (ROT_C below); a float phase would fail that bound by orders of magnitude at first = 2^33.
3. Noise: every sample against the float64 restatement of the rule, per component, under
   2^-23 sigma (NOISE_C1 r + NOISE_C2), which may not exceed 2^-18 sigma; streams repeat and differ as (seed, noise_id) say.
4. Pieces: a carrier made in three calls is bit for bit the carrier made in one.
5. Chirp windows against float64 under the shaper's rotation bound; NULL defaults, guards, _dev = host.
6. Closed loop, all on the device: encode -> mod_shaped + fcch_chirp -> carrier_mix -> rx_run_dev on the same buffer; the
   records are the oracle's on the downloaded samples and are what was sent (tests/carrier_cases.py; the oracle's verdict
   on the inputs alone: tests/test_carrier_host.py).  FCCH acquisition on a chirp-plus-noise carrier.

The bounds.  ROT_C = 5: the phase rounded to float, |theta| <= pi, half an ulp of [2, 4) = 2^-23 rad (1 unit; the double
product adds 2^-52 |cfo n|, carried separately); sincosf within 2 ulp per component of values below 1, 2^-23 each, sqrt(2)
as a vector (1.5 units); the complex product, per component two products and a sum each within 2^-24 relative, as a vector
below 2 units; rounded up.  NOISE_C1 = 4, NOISE_C2 = 1, per component: logf within 2 ulp makes r = sqrtf(-2 logf u1) wrong
by 2^-23 r, sqrtf within 1 ulp by another 2^-23 r (2 units of r); sincospif within 2 ulp, 2^-23 per component (1 unit of
r); the products r c and sigma z, 2^-24 each (1 unit of r together); the sum with acc = 0 is exact.  C2 covers r near 0.
r <= sqrt(-2 ln 2^-24) = 5.77, so the bound stays below 2^-23 sigma 24.1 < 2^-18 sigma."""
import numpy as np
import pytest

import acq_cases as ac
import carrier_cases as cc
import carrier_ref as ref

gpu = pytest.mark.gpu

SENT = np.float32(-7.25)
ROT_C = 5.0
NOISE_C1, NOISE_C2 = 4.0, 1.0
SYM_RATE = 23400


def _guarded(lengths, gaps):
    """carriers of `lengths` in one array with gaps[i] samples in front of carrier i (so offsets of both parities) and a guard
    behind the last: (out filled with SENT, offsets)"""
    off, pos = [], 0
    for ln, g in zip(lengths, gaps):
        pos += g
        off.append(pos)
        pos += ln
    return np.full(2 * (pos + 3), SENT, np.float32).view(np.complex64), np.array(off, np.uint64)


def _inside(out_size, off, lengths):
    m = np.zeros(out_size, bool)
    for o, ln in zip(off, lengths):
        m[int(o):int(o) + int(ln)] = True
    return m


def _flatten(per_carrier):
    """[[(src, pos, len), ...] per carrier] -> seg_first, seg_src, seg_pos, seg_len"""
    first = np.concatenate([[0], np.cumsum([len(s) for s in per_carrier])]).astype(np.int32)
    flat = [s for segs in per_carrier for s in segs]
    col = lambda i, t: np.array([s[i] for s in flat], t)
    return first, col(0, np.uint64), col(1, np.int64), col(2, np.uint32)


# ---- 1. overlap-add, exact ----
def _exact_case(tile):
    """Four carriers in one call: lengths 70 001 (many tiles, odd, odd address, first = 0), 1000 (first = 5000: segments straddle
    its start and its end and lie wholly outside), 1, and 300 without segments."""
    rng = np.random.default_rng(2024)
    seg_iq = (rng.standard_normal(6000) + 1j * rng.standard_normal(6000)).astype(np.complex64)
    seg_iq[0:3] = [1e8, -1e8, 1.0]
    T = tile
    a = [(100, 10, 200), (300, 110, 200),                      # two deep over 110 .. 210
         (500, 150, 100),                                      # three deep over 150 .. 210
         (0, 400, 1), (1, 400, 1), (2, 400, 1),                # the same pos three times: (1e8 + -1e8) + 1 = 1, any other order 0 or 1e8-ish
         (600, 401, 1),                                        # len 1
         (700, 501, 33), (800, 777, 64),                       # odd pos, odd and even source
         (801, 900, 63)]                                       # odd source on an even pos
    for edge in (T, 2 * T, 5 * T):                             # ending on a tile's last sample, starting on the next one's first,
        for d in (-2, -1, 0, 1):                               # for either parity of the carrier's address
            a += [(1000 + 7 * (d + 2), edge + d - 50, 50), (1100 + 5 * (d + 2), edge + d, 50)]
    a += [(2000, 69990, 11), (2100, 69995, 40), (2200, 70001, 10), (2300, -20, 25), (2400, -30, 30)]     # the end, past it, the start
    b = [(3000, 4990, 30), (3100, 4000, 100), (3200, 5990, 30), (3300, 6000, 20), (3400, 5500, 1), (3500, 4999, 1), (3501, 4999, 2)]
    c = [(4000, 0, 1), (4001, 0, 1), (4002, -1, 3), (4010, 1, 5)]
    per = [sorted(s, key=lambda t: t[1]) for s in (a, b, c, [])]          # stable: list order among equal pos stays
    lengths = np.array([70001, 1000, 1, 300], np.uint64)
    first = np.array([0, 5000, 0, 17], np.int64)
    out, off = _guarded(lengths.tolist(), [1, 2, 3, 1])
    assert len(set((off % 2).tolist())) == 2
    return seg_iq, per, lengths, first, out, off


@gpu
def test_overlap_add_is_a_float32_loop_in_list_order(gpu_api):
    import torch
    api = gpu_api
    seg_iq, per, lengths, first, out, off = _exact_case(api.CARRIER_MIX_TILE)
    sf, src, pos, ln = _flatten(per)
    ret = api.carrier_mix(seg_iq, sf, src, pos, ln, lengths, out_offset=off, first=first, out=out)
    assert ret is out
    inside = _inside(out.size, off, lengths)
    assert (out[~inside].view(np.float32) == SENT).all() and (~inside).sum() >= 8           # guards unchanged
    for c in range(4):
        want = ref.overlap_add_f32(seg_iq, per[c], int(first[c]), int(lengths[c]))
        got = out[int(off[c]):int(off[c]) + int(lengths[c])]
        assert got.tobytes() == want.tobytes(), (c, np.flatnonzero(got != want)[:8])
    big = out[int(off[0]):]
    assert big[400] == 1.0 and big[401] == seg_iq[600]                 # list order is visible: (1e8 - 1e8) + 1
    assert not out[int(off[3]):int(off[3]) + 300].any()                # no segments: zeros
    # the device form on the same arrays: the same bytes
    dev = lambda x: torch.from_numpy(x).cuda()
    t = dict(iq=dev(seg_iq.view(np.float32)), sf=dev(sf), src=dev(src.view(np.int64)), pos=dev(pos), ln=dev(ln.view(np.int32)),
             off=dev(off.view(np.int64)), length=dev(lengths.view(np.int64)), first=dev(first))
    t_out = torch.full((2 * out.size,), float(SENT), dtype=torch.float32, device="cuda")
    api.carrier_mix_dev(torch.cuda.current_stream().cuda_stream, 4, t["iq"].data_ptr(), t["sf"].data_ptr(), t["src"].data_ptr(),
                        t["pos"].data_ptr(), t["ln"].data_ptr(), int(ln.max()), t["off"].data_ptr(), t["length"].data_ptr(),
                        int(lengths.max()), t["first"].data_ptr(), None, None, None, 0, t_out.data_ptr())
    torch.cuda.synchronize()
    assert t_out.cpu().numpy().tobytes() == out.tobytes()
    # the fresh-array form: carriers back to back, every sample written
    dense = api.carrier_mix(seg_iq, sf, src, pos, ln, lengths, first=first)
    assert dense.size == int(lengths.sum())
    assert dense[:70001].tobytes() == out[int(off[0]):int(off[0]) + 70001].tobytes()


# ---- 2. rotation ----
def _rot_case(first):
    rng = np.random.default_rng(33)
    seg_iq = (rng.standard_normal(3000) + 1j * rng.standard_normal(3000)).astype(np.complex64)
    segs = [(0, first - 10, 700), (700, first + 300, 900), (1600, first + 900, 800), (2400, first + 2500, 600)]
    return seg_iq, segs, 3001


@gpu
@pytest.mark.parametrize("first", [0, 2 ** 33 + 1], ids=["first0", "first2p33"])
def test_rotation_by_a_double_phase(gpu_api, first):
    seg_iq, segs, length = _rot_case(first)
    cfo = 2 * np.pi * 120.0 / (SYM_RATE * 4)
    sf, src, pos, ln = _flatten([segs])
    got = gpu_api.carrier_mix(seg_iq, sf, src, pos, ln, [length], first=[first], cfo=[cfo]).reshape(-1)
    acc = ref.overlap_add_f32(seg_iq, segs, first, length)             # step 1 is exact (test above): only step 2 is bounded here
    n = first + np.arange(length, dtype=np.int64)
    ph, turns = ref.phase(cfo, n)
    want = acc.astype(np.complex128) * np.exp(1j * ph)
    bound = np.abs(acc) * (2.0 ** -23 * ROT_C + 2.0 ** -52 * turns)
    err = np.abs(got.astype(np.complex128) - want)
    live = bound > 0
    print("first %d: worst error / bound %.3f over %d samples" % (first, (err[live] / bound[live]).max(), live.sum()))
    assert live.sum() > 2000 and (~live).sum() > 100
    assert (err <= bound).all() and not got[~live].any()
    # an implementation with a float phase, restated: at 2^33 it misses the same bound by orders of magnitude
    ph32 = (np.float32(cfo) * n.astype(np.float32)).astype(np.float64)
    err32 = np.abs(acc.astype(np.complex128) * np.exp(1j * ph32) - want)
    if first:
        assert (err32[live] > 1000 * bound[live]).mean() > 0.9
    # cfo = 0 skips the step: the exact sums, not a product with one
    plain = gpu_api.carrier_mix(seg_iq, sf, src, pos, ln, [length], first=[first], cfo=[0.0]).reshape(-1)
    assert plain.tobytes() == acc.tobytes()


# ---- 3. noise ----
def _noise_bound(sigma, r):
    b = 2.0 ** -23 * sigma * (NOISE_C1 * r + NOISE_C2)
    assert b.max() <= 2.0 ** -18 * sigma             # a wrong word moves a sample by the order of sigma: nothing hides under this
    return b


@gpu
@pytest.mark.parametrize("sigma", [1.0, 0.05])
def test_noise_is_the_restated_rule(gpu_api, sigma):
    """Four carrier slots in one call: even and odd first on even and odd addresses (a unit is one Philox pair, or straddles two)"""
    lengths = np.array([4099, 2050, 1, 1030], np.uint64)
    first = np.array([0, 2 ** 33 + 1, 7, 10], np.int64)
    ids = np.array([9, 9, 2 ** 32 - 1, 0], np.uint32)
    out, off = _guarded(lengths.tolist(), [0, 1, 1, 2])
    s32 = np.float32(sigma)
    gpu_api.carrier_mix(None, None, None, None, None, lengths, out_offset=off, first=first, sigma=s32, noise_id=ids, seed=cc.SEED, out=out)
    assert (out[~_inside(out.size, off, lengths)].view(np.float32) == SENT).all()
    worst = 0.0
    for c in range(4):
        n = int(first[c]) + np.arange(int(lengths[c]), dtype=np.int64)
        z, r = ref.noise(cc.SEED, int(ids[c]), n)
        want = float(s32) * z
        got = out[int(off[c]):int(off[c]) + int(lengths[c])].astype(np.complex128)
        bound = _noise_bound(float(s32), r)
        for e in (np.abs(got.real - want.real), np.abs(got.imag - want.imag)):
            worst = max(worst, (e / bound).max())
            assert (e <= bound).all(), (c, np.flatnonzero(e > bound)[:5])
    print("sigma %g: worst error / bound %.3f" % (sigma, worst))


@gpu
def test_noise_streams_repeat_and_differ_as_seed_and_id_say(gpu_api):
    api = gpu_api
    run = lambda ids, seed, first=0: api.carrier_mix(None, None, None, None, None, [515, 515], first=first, sigma=1.0, noise_id=ids,
                                                     seed=seed)
    a = run([4, 4], 77)
    assert a.shape == (2, 515) and a[0].tobytes() == a[1].tobytes() and a.any()      # two slots, one stream
    assert run([4, 5], 77)[0].tobytes() == a[0].tobytes()                                    # another call
    b = run([4, 5], 78)
    assert not (run([4, 5], 77)[1] == a[0]).any() and not (b[0] == a[0]).any()               # another id, another seed
    # NULL noise_id: the carrier's index
    c = api.carrier_mix(None, None, None, None, None, [515, 515], sigma=1.0, seed=77)
    assert c.tobytes() == run([0, 1], 77).tobytes()
    # the stream is a function of the absolute index
    assert run([4, 4], 77, first=[0, 101])[1][:414].tobytes() == a[0][101:].tobytes()


# ---- 4. pieces ----
@gpu
def test_a_carrier_made_in_pieces_is_the_carrier_made_in_one_call(gpu_api):
    """Segments, cfo and sigma; cut at an odd and at an even index, both through one segment; the pieces lie at other
    addresses (parities) than the samples had in the whole."""
    rng = np.random.default_rng(44)
    seg_iq = (rng.standard_normal(4000) + 1j * rng.standard_normal(4000)).astype(np.complex64)
    base = 2 ** 33 + 5
    segs = [(0, base - 40, 100), (100, base + 500, 2500), (2600, base + 700, 300), (2900, base + 2950, 1000)]
    length, cuts = 3500, (1237, 2400)
    assert segs[1][1] < base + cuts[0] < base + cuts[1] < segs[1][1] + segs[1][2]
    sf, src, pos, ln = _flatten([segs])
    kw = dict(sigma=[0.3], cfo=[-2 * np.pi * 300.0 / (SYM_RATE * 4)], noise_id=[11], seed=cc.SEED)
    whole = gpu_api.carrier_mix(seg_iq, sf, src, pos, ln, [length], first=[base], **kw).reshape(-1)
    edges = (0,) + cuts + (length,)
    out = np.full(2 * (length + 8), SENT, np.float32).view(np.complex64)
    at = 1
    for lo, hi in zip(edges[:-1], edges[1:]):
        gpu_api.carrier_mix(seg_iq, sf, src, pos, ln, [hi - lo], out_offset=[at], first=[base + lo], out=out, **kw)
        assert out[at:at + hi - lo].tobytes() == whole[lo:hi].tobytes(), (lo, hi)
        at += hi - lo + 1
    # and the whole is the restatement of steps 2 and 3 on the exact sums, to the sum of their bounds and the last addition's
    acc = ref.overlap_add_f32(seg_iq, segs, base, length)
    n = base + np.arange(length, dtype=np.int64)
    ph, turns = ref.phase(kw["cfo"][0], n)
    z, r = ref.noise(cc.SEED, 11, n)
    s32 = float(np.float32(0.3))
    want = acc.astype(np.complex128) * np.exp(1j * ph) + s32 * z
    bound = np.abs(acc) * (2.0 ** -23 * ROT_C + 2.0 ** -52 * turns) + np.sqrt(2.0) * _noise_bound(s32, r) + 2.0 ** -23 * np.abs(want)
    assert (np.abs(whole - want) <= bound).all()


# ---- 5. chirp windows ----
def _chirp_want(freq, length, sps, in_len, start, frac, cfo, phase0, gain):
    """The header's formula in float64 -> (windows (n, in_len) complex128, the bound per sample): the chirp value in double
    rounded to float once (2^-24 relative, and 2^-40 absolute for the device's own double cos), then the shaper's rotation:
    two roundings of the phase, sincosf, the products (tests/test_gpu_mod_shaped.py: 2^-23 (2 |phase| + 4) |body|)."""
    n = len(start)
    k = np.arange(in_len, dtype=np.int64)
    x = np.zeros((n, in_len), np.complex128)
    bound = np.zeros((n, in_len))
    for b in range(n):
        q = k - int(start[b])
        ok = (q >= 0) & (q < length * sps)
        t = (q[ok] - float(frac[b])) / sps - length / 2.0
        v = np.sqrt(2.0) * np.cos(freq * 2 * np.pi / length * t * t)
        ph = float(phase0[b]) + float(cfo[b]) * k[ok]
        x[b, ok] = float(gain[b]) * np.exp(1j * ph) * v
        bound[b, ok] = float(gain[b]) * (2.0 ** -23 * (2 * np.abs(ph) + 5) * np.abs(v) + 2.0 ** -40)
    return x, bound


CHIRP_CELLS = [(t, sps) for t in ("fcch", "fcch3_lband", "fcch3_sband") for sps in (1, 4, 16)]


@gpu
@pytest.mark.parametrize("fcch_type,sps", CHIRP_CELLS, ids=lambda v: str(v))
def test_chirp_windows_against_float64(gpu_api, fcch_type, sps):
    import torch
    api = gpu_api
    d = api.FcchBurst.in_dll(api.load(), {"fcch": "gmr1_fcch_burst", "fcch3_lband": "gmr1_fcch3_lband_burst",
                                          "fcch3_sband": "gmr1_fcch3_sband_burst"}[fcch_type])
    freq, length = float(d.freq), int(d.len)
    assert length == ac.BURST_LEN[fcch_type] and freq == float(np.float32({"fcch3_sband": 0.16}.get(fcch_type, 0.32)))      # fcch.c:52-70
    body = length * sps
    in_len = body + 7
    rng = np.random.default_rng(60 + sps)
    # frac 0 and 0.37; the chirp inside, clipped at the left (start < 0) and at the right
    start = np.array([3, 4, -(body // 3), in_len - body // 2, 0, in_len + 5], np.int32)
    frac = np.array([0.0, 0.37, 0.37, 0.0, 0.37, 0.0], np.float32)
    n = start.size
    cfo = (rng.normal(0.0, 150.0, n) * (2 * np.pi / (SYM_RATE * sps))).astype(np.float32)
    ph0 = rng.uniform(0, 2 * np.pi, n).astype(np.float32)
    gain = (10.0 ** (rng.normal(0.0, 3.0, n) / 20.0)).astype(np.float32)
    off = (np.cumsum(np.arange(1, n + 1) % 4 + in_len) - in_len).astype(np.uint64)           # gaps 1, 2, 3, 0: both parities
    out_len = int(off[-1]) + in_len + 5
    assert len(set((off % 2).tolist())) == 2
    out = np.full(2 * out_len, SENT, np.float32).view(np.complex64)
    imp = dict(start=start, frac=frac, cfo=cfo, phase0=ph0, gain=gain)
    assert api.fcch_chirp_batch(n, sps, in_len, fcch_type=fcch_type, offset=off, out=out, **imp) is out
    inside = _inside(out_len, off, [in_len] * n)
    assert (out[~inside].view(np.float32) == SENT).all() and not (out[inside].view(np.float32) == SENT).any()
    want, bound = _chirp_want(freq, length, sps, in_len, **imp)
    win = np.stack([out[int(o):int(o) + in_len] for o in off])
    err = np.abs(win - want)
    live = bound > 0
    print("%s sps %d: worst error / bound %.3f" % (fcch_type, sps, (err[live] / bound[live]).max()))
    assert live[2, 0] and not live[2, -1] and live[3, -1] and not live[3, 0] and not live[5].any() and live[:5].any(1).all()
    assert not win[~live].any() and (err <= bound).all()
    # wherever the windows lie: the dense form gives the same windows
    assert api.fcch_chirp_batch(n, sps, in_len, fcch_type=fcch_type, **imp).tobytes() == win.tobytes()
    # NULL = 0, 0, 0, 0, 1, and then the window is synth's chirp (here: its formula in float64, rounded once)
    none = api.fcch_chirp_batch(2, sps, in_len, fcch_type=fcch_type)
    z, one = np.zeros(2, np.float32), np.ones(2, np.float32)
    given = api.fcch_chirp_batch(2, sps, in_len, fcch_type=fcch_type, start=np.zeros(2, np.int32), frac=z, cfo=z, phase0=z, gain=one)
    assert none.tobytes() == given.tobytes() and not none.imag.any() and not none[:, body:].any()
    t = np.arange(body) / sps - length / 2.0
    plain = (np.sqrt(2.0) * np.cos(freq * 2 * np.pi / length * t * t))
    assert np.abs(none[0, :body].real - plain).max() <= 2.0 ** -23 * np.sqrt(2.0) + 2.0 ** -40
    # the device form: the kernel itself leaves the gaps alone
    dev = lambda a: torch.from_numpy(a).cuda()
    tt = dict(off=dev(off.view(np.int64)), **{k: dev(v) for k, v in imp.items()})
    t_out = torch.full((2 * out_len,), float(SENT), dtype=torch.float32, device="cuda")
    api.fcch_chirp_batch_dev(torch.cuda.current_stream().cuda_stream, fcch_type, n, sps, in_len, tt["off"].data_ptr(),
                             tt["start"].data_ptr(), tt["frac"].data_ptr(), tt["cfo"].data_ptr(), tt["phase0"].data_ptr(),
                             tt["gain"].data_ptr(), t_out.data_ptr(), out_len)
    torch.cuda.synchronize()
    assert t_out.cpu().numpy().tobytes() == out.tobytes()


# ---- 6. the closed loop, all on the device ----
def _key(rec):
    """the key of tests/test_gpu_rxloop.py"""
    return [(int(r["arfcn"]), int(r["chain"]), int(r["type"]), int(r["fn"]), int(r["tn"]), bytes(r["l2"])) for r in rec]


def _carrier_on_device(api, torch, b):
    """encode -> mod_shaped / fcch_chirp -> carrier_mix, every array in device memory -> the carrier (a float32 cuda tensor)"""
    st = torch.cuda.current_stream().cuda_stream
    sps = b["sps"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    seg_iq = torch.zeros(2 * b["seg_iq_len"], dtype=torch.float32, device="cuda")
    keep = []
    for kind, fmt, enc, nbits in (("bcch", "bcch", "gmr1_hip_bcch_encode_batch_dev", 424), ("ccch", "dc6", "gmr1_hip_ccch_encode_batch_dev", 432)):
        k = b["kinds"][kind]
        l2 = dev(k["l2"])
        ebits = torch.zeros(k["n"] * nbits, dtype=torch.uint8, device="cuda")
        api._call(enc, st, k["n"], l2.data_ptr(), ebits.data_ptr())
        off = dev((k["base"] + np.arange(k["n"], dtype=np.int64) * k["in_len"]))
        start = dev(np.full(k["n"], cc.SPAN * sps, np.int32))
        gain = dev(k["gain"])
        api.mod_shaped_batch_dev(st, fmt, k["n"], sps, api.PULSE_RC, cc.SPAN, k["in_len"], ebits.data_ptr(), None, off.data_ptr(),
                                 start.data_ptr(), None, None, None, gain.data_ptr(), seg_iq.data_ptr(), b["seg_iq_len"])
        keep += [l2, ebits, off, start, gain]
    k = b["kinds"]["fcch"]
    off = dev((k["base"] + np.arange(k["n"], dtype=np.int64) * k["in_len"]))
    gain = dev(k["gain"])
    api.fcch_chirp_batch_dev(st, "fcch", k["n"], sps, k["in_len"], off.data_ptr(), None, None, None, None, gain.data_ptr(),
                             seg_iq.data_ptr(), b["seg_iq_len"])
    n_seg = b["seg_pos"].size
    t = dict(sf=dev(np.array([0, n_seg], np.int32)), src=dev(b["seg_src"].view(np.int64)), pos=dev(b["seg_pos"]),
             ln=dev(b["seg_len"].view(np.int32)), off=dev(np.zeros(1, np.int64)), length=dev(np.array([b["n"]], np.int64)),
             sigma=dev(np.array([b["sigma"]], np.float32)), cfo=dev(np.array([b["cfo"]], np.float64)),
             nid=dev(np.array([b["noise_id"]], np.uint32).view(np.int32)))
    x = torch.zeros(2 * b["n"], dtype=torch.float32, device="cuda")
    api.carrier_mix_dev(st, 1, seg_iq.data_ptr(), t["sf"].data_ptr(), t["src"].data_ptr(), t["pos"].data_ptr(), t["ln"].data_ptr(),
                        int(b["seg_len"].max()), t["off"].data_ptr(), t["length"].data_ptr(), b["n"], None, t["sigma"].data_ptr(),
                        t["cfo"].data_ptr(), t["nid"].data_ptr(), b["seed"], x.data_ptr())
    torch.cuda.synchronize()
    return x


@gpu
@pytest.mark.parametrize("name", list(cc.CASES))
def test_closed_loop_on_the_device(gpu_api, orc, pkg, name):
    import torch
    api = gpu_api
    b = cc.build(pkg, name)
    x = _carrier_on_device(api, torch, b)
    rec, status, chains, found = api.rx_run_dev(torch.cuda.current_stream().cuda_stream, x.data_ptr(), [0], [b["n"]], sps=b["sps"])
    assert status[0] == 0 and found == len(rec)
    host = x.cpu().numpy().view(np.complex64)
    orv, orec, och = orc.rx_run(host, sps=b["sps"], arfcn=0)
    assert orv == 0 and chains[0] == och
    assert _key(rec) == _key(orec), "the records differ from the oracle's on the same samples"
    v = cc.check_records(rec, int(chains[0]), b)
    print(name, "chains", int(chains[0]), "records", len(rec), v)
    if name == "two_tx":
        assert chains[0] > 1 and all(k[1] for k in v)
    # and the samples are the restatement's carrier to within the noise floor's own rounding and the windows': far below sigma
    want = cc.restate(pkg, b)
    assert np.abs(host - want).max() < 1e-3 * b["sigma"] + 1e-4


@gpu
def test_fcch_acquisition_on_a_chirp_plus_noise_carrier(gpu_api, orc):
    """FCCH chirps every 320 ms over noise of variance 1 per complex sample at 6 dB, 100 Hz off (synth_fcch_stream's
    stream, made by the chirp entry and the mixer): the acquisition's record is the oracle's under the tolerances of
    tests/test_gpu_fcch_acquire.py (chain_align equal), and every chain_align lies within one symbol of a transmitted chirp
    position (the fine stage resolves single samples; a symbol is what its search covers either way)."""
    api = gpu_api
    sps, n = ac.SPS, ac.N_15
    period, first_chirp, flen = 7488 * sps, 3000, 117 * sps
    pos = np.arange(first_chirp, n - flen, period, dtype=np.int64)
    amp = np.float32(10.0 ** (6.0 / 20.0))
    chirps = api.fcch_chirp_batch(pos.size, sps, flen, gain=amp).reshape(-1)
    x = api.carrier_mix(chirps, [0, pos.size], np.arange(pos.size) * flen, pos, np.full(pos.size, flen), [n],
                        sigma=np.sqrt(0.5), cfo=2 * np.pi * 100.0 / (SYM_RATE * sps), noise_id=21, seed=cc.SEED).reshape(-1)
    got = api.fcch_acquire(x, [0], [n], sps=sps)[0]
    want, margins = ac.expected(orc, x, sps, 8000, "fcch")
    assert all(min(m) >= ac.MARGIN for m in margins)
    assert int(got["status"]) == int(want["status"]) == 0 and int(got["n_chains"]) == int(want["n_chains"]) >= 1
    assert list(got["chain_align"]) == list(want["chain_align"])
    for k in ("align", "base_align", "n_cand"):
        assert int(got[k]) == int(want[k]), k
    assert abs(float(got["freq_err"]) - float(want["freq_err"])) < 1e-4
    for j in range(int(got["n_chains"])):
        assert abs(float(got["chain_freq_err"][j]) - float(want["chain_freq_err"][j])) < 1e-4
        assert abs(float(got["chain_snr"][j]) - float(want["chain_snr"][j])) <= 2e-4 * max(1.0, abs(float(want["chain_snr"][j])))
        d = np.abs(int(got["chain_align"][j]) - pos).min()
        print("chain %d: align %d, %d samples from a transmitted chirp" % (j, int(got["chain_align"][j]), d))
        assert d <= sps
