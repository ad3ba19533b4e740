"""GPU tests of the integer IQ entries (gmr1_hip_*_iq*): an int16 or int8 capture, read by the first kernel of the chain
itself, must give BIT FOR BIT (np.array_equal) what the float entry gives on its float twin  x.astype(float32) * 2^-k  --
the conversion is exact, so there is nothing to tolerate -- one-shot, through pointers one sample into an allocation, and
streamed in pieces of any size; and, so that the feature is not only tested against its sibling, what oracle/orc_chan.py
computes from the twin, within the channelizer's 2e-4 contract (tests/test_gpu_chan.py).

Captures are test_gpu_chan_stream._capture's (noise and three tones), scaled so that they fill about a quarter of the
integer range and rounded; the first eight samples are the extremes (the type's minimum, its maximum, -1, 0, 1) in both
components."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from test_gpu_chan_stream import CHANS, FS, _capture, _random_sizes, _streamed

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu

FMTS = {"s16": (np.int16, 15), "s8": (np.int8, 7)}
FREQS = [3 * 31250.0, -7 * 31250.0 + 400.0, 0.0]           # test_direct_mode_streams_bit_identically's
N_FB = 100000 + 7
N_DIRECT = 200000 + 13
N_SPS = 150000 + 3


@functools.lru_cache(maxsize=None)
def _pair(name, n, fs, seed, n_chans=64):
    """-> (the integer capture (n, 2), its float twin complex64 (n,)); computed once, never written to"""
    dtype, k = FMTS[name]
    info = np.iinfo(dtype)
    x = _capture(n, fs, seed, n_chans).view(np.float32).reshape(n, 2)
    q = np.rint(x * (0.25 * 2.0 ** k / np.abs(x).max())).astype(dtype)
    lo, hi = info.min, info.max
    q[:8, 0] = [lo, hi, -1, 0, 1, lo, hi, 0]
    q[:8, 1] = [hi, lo, 1, 0, -1, lo, hi, -1]
    twin = (q.astype(np.float32) * np.float32(2.0 ** -k)).view(np.complex64).reshape(-1)
    assert twin[0] == np.complex64(complex(-1.0, hi * 2.0 ** -k))
    assert 0.2 * 2 ** k < np.abs(q[8:].astype(np.int32)).max() <= 0.25 * 2 ** k + 1
    q.setflags(write=False)
    twin.setflags(write=False)
    return q, twin


def _fmt(api, name):
    return {"s16": api.IQ_S16, "s8": api.IQ_S8}[name]


def _fb_case(api, fs):
    """(n, channels) of a filterbank rate: the fast path's case, or the generic / off-grid ones of the streaming tests"""
    if fs == FS:
        return N_FB, CHANS, 64
    M, _, _ = api.channelize_plan(fs, 4, 0)
    return 40 * M * 50 + 37, [3, M - 2, M // 2 - 1, 0, M - 1, M // 2], M


_ONE_SHOT = {}


def _one_shot(api, name, fs, rot=0.0):
    """case 1's integer one-shot output, computed once per (format, rate, rotation)"""
    key = (name, fs, rot)
    if key not in _ONE_SHOT:
        n, chans, M = _fb_case(api, fs)
        q, _ = _pair(name, n, fs, int(fs) % 1000 + 5, M)
        _ONE_SHOT[key] = api.channelize_iq(q, fs, chans, rotation=rot)
    return _ONE_SHOT[key]


def _one_shot_direct(api, name, fs):
    key = (name, fs, "direct")
    if key not in _ONE_SHOT:
        q, _ = _pair(name, N_DIRECT, fs, int(fs) % 97)
        _ONE_SHOT[key] = api.ddc_iq(q, fs, FREQS)
    return _ONE_SHOT[key]


# ---- 1. one-shot, bit-identical to the float entry ------------------------------------------------------------------
@pytest.mark.parametrize("rot", [0.0, 0.21])
@pytest.mark.parametrize("fs", [2.0e6, 1.0e6, 1.25e6, 2.048e6])
@pytest.mark.parametrize("name", list(FMTS))
def test_filterbank_one_shot_equals_the_float_entry(gpu_api, name, fs, rot):
    """2.0 Msps: k_pfb64; 1.0 and 1.25: k_pfb_any (32 and 40 channels); 2.048: off the grid, the converting path"""
    n, chans, M = _fb_case(gpu_api, fs)
    _, twin = _pair(name, n, fs, int(fs) % 1000 + 5, M)
    got = _one_shot(gpu_api, name, fs, rot)
    ref = gpu_api.channelize(twin, fs, chans, rotation=rot)
    assert got.shape == ref.shape and ref.shape[1] > 0
    assert np.abs(ref).max() > 0
    assert np.array_equal(got, ref), (name, fs, rot)


@pytest.mark.parametrize("name", list(FMTS))
def test_planar_entry_equals_the_float_planar_entry(gpu_api, name):
    import torch
    q, twin = _pair(name, N_FB, FS, 5)
    _, _, n_out = gpu_api.channelize_plan(FS, 4, N_FB)
    stride = n_out + 7
    P = -(-len(CHANS) * stride // 4) + 2
    tq = torch.from_numpy(np.array(q)).cuda()
    tf = torch.from_numpy(np.array(twin).view(np.float32)).cuda()
    planes = [torch.zeros((4 * P, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
    w = gpu_api.channelize_planar_iq_dev(None, _fmt(gpu_api, name), tq.data_ptr(), N_FB, FS, CHANS, planes[0].data_ptr(), stride, P)
    assert w == n_out
    assert gpu_api.channelize_planar_dev(None, tf.data_ptr(), N_FB, FS, CHANS, planes[1].data_ptr(), stride, P) == n_out
    torch.cuda.synchronize()
    a, b = planes[0].cpu().numpy(), planes[1].cpu().numpy()
    assert np.abs(b).max() > 0
    assert np.array_equal(a, b)


@pytest.mark.parametrize("fs", [2.0e6, 1.25e6, 1.0e6])
@pytest.mark.parametrize("name", list(FMTS))
def test_direct_mode_one_shot_equals_the_float_entry(gpu_api, name, fs):
    _, twin = _pair(name, N_DIRECT, fs, int(fs) % 97)
    got = _one_shot_direct(gpu_api, name, fs)
    ref = gpu_api.ddc(twin, fs, FREQS)
    assert got.shape == ref.shape and ref.shape[1] > 0 and np.abs(ref).max() > 0
    assert np.array_equal(got, ref), (name, fs)


@pytest.mark.parametrize("sps", [1, 2])
@pytest.mark.parametrize("name", list(FMTS))
def test_other_sps_both_modes(gpu_api, name, sps):
    q, twin = _pair(name, N_SPS, FS, 8)
    got, ref = gpu_api.channelize_iq(q, FS, [5, 31], sps=sps), gpu_api.channelize(twin, FS, [5, 31], sps=sps)
    assert got.shape == ref.shape and ref.shape[1] > 0
    assert np.array_equal(got, ref)
    got, ref = gpu_api.ddc_iq(q, FS, [31250.0], sps=sps), gpu_api.ddc(twin, FS, [31250.0], sps=sps)
    assert got.shape == ref.shape and ref.shape[1] > 0
    assert np.array_equal(got, ref)


# ---- 2. against the numpy restatement, not only the sibling ---------------------------------------------------------
@pytest.mark.parametrize("name", list(FMTS))
def test_integer_capture_matches_oracle(gpu_api, name):
    """the bound of test_channelizer_matches_oracle for this plan: the project's 2e-4 contract"""
    import orc_chan
    pl = orc_chan.Plan(FS)
    _, twin = _pair(name, N_FB, FS, 5)
    got = _one_shot(gpu_api, name, FS)
    ref = orc_chan.channelize(np.array(twin), pl, CHANS)
    for i, k in enumerate(CHANS):
        r = ref[k]
        assert got[i].size == r.size
        err = np.max(np.abs(got[i] - r))
        print(name, "channel", k, "max error", err, "rms", float(np.sqrt(np.mean(np.abs(r) ** 2))))
        assert err < 2e-4 * max(1.0, float(np.sqrt(np.mean(np.abs(r) ** 2)))), (k, err)


# ---- 3. pointers one sample into an allocation ----------------------------------------------------------------------
def _one_in(q):
    """a device buffer holding the capture one sample in -> (tensor, pointer to the capture: 4 B off for S16, 2 B for S8)"""
    import torch
    t = torch.zeros((q.shape[0] + 1, 2), dtype=torch.from_numpy(np.array(q[:1])).dtype, device="cuda")
    t[1:] = torch.from_numpy(np.array(q)).cuda()
    return t, t.data_ptr() + 2 * q.dtype.itemsize


@pytest.mark.parametrize("name", list(FMTS))
def test_unaligned_device_pointers(gpu_api, name):
    import torch
    fmt = _fmt(gpu_api, name)
    q, _ = _pair(name, N_FB, FS, 5)
    t, ptr = _one_in(q)
    assert ptr % (2 * q.dtype.itemsize) == 0 and ptr % (4 * q.dtype.itemsize) != 0
    want = _one_shot(gpu_api, name, FS)
    out = torch.zeros((len(CHANS), want.shape[1], 2), dtype=torch.float32, device="cuda")
    assert gpu_api.channelize_iq_dev(None, fmt, ptr, N_FB, FS, CHANS, out.data_ptr(), want.shape[1]) == want.shape[1]
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.complex64).reshape(want.shape), want)
    q, _ = _pair(name, N_DIRECT, FS, int(FS) % 97)
    t, ptr = _one_in(q)
    want = _one_shot_direct(gpu_api, name, FS)
    out = torch.zeros((len(FREQS), want.shape[1], 2), dtype=torch.float32, device="cuda")
    assert gpu_api.ddc_iq_dev(None, fmt, ptr, N_DIRECT, FS, FREQS, out.data_ptr(), want.shape[1]) == want.shape[1]
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.complex64).reshape(want.shape), want)


# ---- 4. streaming ---------------------------------------------------------------------------------------------------
def _streamed_iq(api, cs, q, sizes, fs, direct):
    """host pushes of q in pieces of `sizes`; every push's count is out_len's and the plan's n_out(N + n) - n_out(N)"""
    plan = (lambda n: api.ddc_plan(fs, 4, n)[3]) if direct else (lambda n: api.channelize_plan(fs, 4, n)[2])
    outs, pos = [], 0
    for k in sizes:
        want = plan(pos + k) - plan(pos)
        assert cs.out_len(k) == want, (pos, k)
        o = cs.push(q[pos:pos + k])
        assert o.shape == (cs.n_sel, want), (pos, k, o.shape, want)
        outs.append(o)
        pos += k
    assert pos == q.shape[0]
    return np.concatenate(outs, axis=1)


def _streamed_iq_dev(api, cs, q, sizes, n_out):
    """the same pieces as device pointers into ONE buffer: a piece starts where the last one ended, so after an odd count
    an S8 piece is 2-byte aligned and no more"""
    import torch
    t = torch.from_numpy(np.array(q)).cuda()
    out = torch.zeros((cs.n_sel, n_out, 2), dtype=torch.float32, device="cuda")
    sb, pos, done = 2 * q.dtype.itemsize, 0, 0
    for k in sizes:
        want = cs.out_len(k)
        got = cs.push_dev(None, t.data_ptr() + sb * pos, k, out.data_ptr() + 8 * done, n_out)
        assert got == want, (pos, k)
        pos += k
        done += got
    torch.cuda.synchronize()
    assert done == n_out
    return out.cpu().numpy().view(np.complex64).reshape(cs.n_sel, n_out)


@pytest.mark.parametrize("mode,fs", [("fb", 2.0e6), ("fb", 1.25e6), ("fb", 2.048e6), ("direct", 2.0e6), ("direct", 1.0e6)])
@pytest.mark.parametrize("name", list(FMTS))
def test_streamed_equals_one_shot_and_the_float_stream(gpu_api, name, mode, fs):
    api, fmt, direct = gpu_api, _fmt(gpu_api, name), mode == "direct"
    if direct:
        n, sel = N_DIRECT, FREQS
        q, twin = _pair(name, n, fs, int(fs) % 97)
        want = _one_shot_direct(api, name, fs)
        make = lambda f: api.ChanStream.direct(fs, sel, fmt=f)         # noqa: E731
    else:
        n, sel, M = _fb_case(api, fs)
        q, twin = _pair(name, n, fs, int(fs) % 1000 + 5, M)
        want = _one_shot(api, name, fs)
        make = lambda f: api.ChanStream(fs, sel, fmt=f)                # noqa: E731
    sizes = _random_sizes(n, int(fs) % 77 + len(name), hi=n // 5)
    assert any(k % 2 for k in sizes[:-1])
    with make(fmt) as cs:
        got = _streamed_iq(api, cs, q, sizes, fs, direct)
    assert got.shape == want.shape
    assert np.array_equal(got, want), "host pushes against the one-shot integer call"
    with make(fmt) as cs:
        got = _streamed_iq_dev(api, cs, q, sizes, want.shape[1])
    assert np.array_equal(got, want), "device pushes against the one-shot integer call"
    with make(api.IQ_F32) as cs:
        flt = _streamed(api, cs, twin, sizes, fs, direct=direct)
    assert np.array_equal(flt, want), "the float stream on the twin"


# ---- 5. a handle's format, and refusals -----------------------------------------------------------------------------
def _raw_push(lib, fn, cs, chunk, out):
    got = C.c_uint64(0)
    n = chunk.shape[0]
    rc = getattr(lib, fn)(cs._h, chunk.ctypes.data_as(C.c_void_p), C.c_uint64(n), out.ctypes.data_as(C.c_void_p),
                          C.c_uint64(out.shape[1]), C.byref(got))
    return rc, got.value


def test_float_push_on_an_integer_handle_is_refused_and_leaves_it_as_it_was(gpu_api):
    lib = gpu_api.load()
    q, twin = _pair("s16", N_FB, FS, 5)
    want = _one_shot(gpu_api, "s16", FS)
    with gpu_api.ChanStream(FS, CHANS, fmt=gpu_api.IQ_S16) as cs:
        a = cs.push(q[:30001])
        k = 20000
        need = cs.out_len(k)
        assert need > 0
        out = np.zeros((len(CHANS), need), np.complex64)
        chunk = np.ascontiguousarray(twin[30001:30001 + k])
        rc, _ = _raw_push(lib, "gmr1_hip_chan_stream_push", cs, chunk, out)
        assert rc == -22
        assert cs.out_len(k) == need                                    # nothing was counted
        with pytest.raises(TypeError):
            cs.push(chunk)                                              # the mirror says so before the library is asked
        b = cs.push(q[30001:])
    assert np.array_equal(np.concatenate([a, b], axis=1), want)


def test_push_iq_on_a_plain_handle_equals_push(gpu_api):
    lib = gpu_api.load()
    _, twin = _pair("s16", N_FB, FS, 5)
    ref = gpu_api.channelize(twin, FS, CHANS)
    outs = []
    with gpu_api.ChanStream(FS, CHANS) as cs:                           # gmr1_hip_channelize_stream_create_iq(F32) underneath
        assert cs.fmt == gpu_api.IQ_F32
    h = C.c_void_p()
    ch = np.array(CHANS, np.int32)
    assert lib.gmr1_hip_channelize_stream_create(C.c_double(FS), 4, C.c_float(0.0), ch.size, ch.ctypes.data_as(C.c_void_p),
                                                 C.byref(h)) == 0
    cs = gpu_api.ChanStream(None, None, _handle=h, _n_sel=ch.size)      # a handle of the existing _create
    with cs:
        pos = 0
        for j, k in enumerate((40001, 9, 30000, N_FB - 70010)):
            chunk = np.ascontiguousarray(twin[pos:pos + k])
            out = np.zeros((ch.size, max(cs.out_len(k), 1)), np.complex64)
            fn = "gmr1_hip_chan_stream_push_iq" if j % 2 == 0 else "gmr1_hip_chan_stream_push"
            rc, got = _raw_push(lib, fn, cs, chunk, out)
            assert rc == 0
            outs.append(out[:, :got])
            pos += k
    assert np.array_equal(np.concatenate(outs, axis=1), ref)


def test_unknown_format_is_refused_everywhere(gpu_api):
    import torch
    lib, api = gpu_api.load(), gpu_api
    q, _ = _pair("s16", N_FB, FS, 5)
    t = torch.from_numpy(np.array(q)).cuda()
    out = torch.zeros((len(CHANS), 8000, 2), dtype=torch.float32, device="cuda")
    ch, fr = np.array(CHANS, np.int32), np.array(FREQS, np.float64)
    host_out = np.zeros((len(CHANS), 8000), np.complex64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                          # noqa: E731
    d, f, u = C.c_double(FS), C.c_float(0.0), C.c_uint64
    dq, do = C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())
    h = C.c_void_p()
    for fmt in (3, -1):
        assert lib.gmr1_hip_channelize_iq_dev(None, d, 4, fmt, dq, u(N_FB), f, ch.size, p(ch), do, u(8000), None) == -22
        assert lib.gmr1_hip_channelize_iq(d, 4, fmt, p(q), u(N_FB), f, ch.size, p(ch), p(host_out), u(8000), None) == -22
        assert lib.gmr1_hip_channelize_planar_iq_dev(None, d, 4, fmt, dq, u(N_FB), f, ch.size, p(ch), do, u(8000), u(16000),
                                                     None) == -22
        assert lib.gmr1_hip_ddc_iq_dev(None, d, 4, fmt, dq, u(N_FB), fr.size, p(fr), do, u(8000), None) == -22
        assert lib.gmr1_hip_ddc_iq(d, 4, fmt, p(q), u(N_FB), fr.size, p(fr), p(host_out), u(8000), None) == -22
        assert lib.gmr1_hip_channelize_stream_create_iq(d, 4, fmt, f, ch.size, p(ch), C.byref(h)) == -22
        assert lib.gmr1_hip_ddc_stream_create_iq(d, 4, fmt, fr.size, p(fr), C.byref(h)) == -22
        assert not h.value
    with pytest.raises(api.Gmr1HipError, match="-22"):
        api.ChanStream(FS, CHANS, fmt=3)
    with pytest.raises(api.Gmr1HipError, match="-22"):
        api.ChanStream.direct(FS, FREQS, fmt=3)


def test_no_samples_is_accepted_in_every_format(gpu_api):
    api = gpu_api
    empty = {api.IQ_F32: np.zeros(0, np.complex64), api.IQ_S16: np.zeros((0, 2), np.int16), api.IQ_S8: np.zeros((0, 2), np.int8)}
    for fmt, x in empty.items():
        assert api.channelize_iq(x, FS, CHANS).shape == (len(CHANS), 0)
        assert api.ddc_iq(x, FS, FREQS).shape == (len(FREQS), 0)
        with api.ChanStream(FS, CHANS, fmt=fmt) as cs:
            assert cs.push(x).shape == (len(CHANS), 0)
        with api.ChanStream.direct(FS, FREQS, fmt=fmt) as cs:
            assert cs.push(x).shape == (len(FREQS), 0)
