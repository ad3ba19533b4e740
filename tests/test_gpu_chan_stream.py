"""GPU tests of the streaming channelizer (gmr1_hip_channelize_stream_create / gmr1_hip_ddc_stream_create and
gmr1_hip_chan_stream_*): a capture pushed piece by piece must give, concatenated, exactly what one one-shot call on the
whole capture gives (np.array_equal), whatever the chunk sizes."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 2.0e6
CHANS = [5, 40, 31, 0, 63, 32]
SPECIAL = [0, 1, 31, 32, 33, 63, 64, 65]


def _capture(n, fs, seed, n_chans=64):
    """noise plus three tones on channels 5, 40 and 31 (as test_channelizer_matches_oracle)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 2)) * 0.3).astype(np.float32).view(np.complex64).reshape(-1)
    s = np.arange(n, dtype=np.float64)
    for k, f, a in ((5, 1000.0, 1.0), (n_chans - 24, -4000.0, 0.5), (n_chans // 2 - 1, 9000.0, 2.0)):
        kk = k if k < n_chans // 2 else k - n_chans
        ph = np.mod(((kk * 31250.0 + f) / fs) * s, 1.0)
        x += (a * np.exp(2j * np.pi * ph)).astype(np.complex64)
    return x


def _random_sizes(n, seed, hi=300000):
    """chunk sizes between 0 and hi summing to n, each of SPECIAL among them"""
    rng = np.random.default_rng(seed)
    sizes = list(SPECIAL)
    while sum(sizes) < n:
        sizes.append(int(rng.integers(0, hi + 1)))
    rng.shuffle(sizes)
    out, left = [], n
    for k in sizes:
        k = min(k, left)
        out.append(k)
        left -= k
    out.append(left)
    return out


def _plan_out(api, direct, fs, n, sps=4):
    return api.ddc_plan(fs, sps, n)[3] if direct else api.channelize_plan(fs, sps, n)[2]


def _streamed(api, cs, x, sizes, fs, direct=False, sps=4):
    """push x in pieces of `sizes`; every push's count checked against out_len and the plan's n_out(N + n) - n_out(N)"""
    outs, pos = [], 0
    for k in sizes:
        want = _plan_out(api, direct, fs, pos + k, sps) - _plan_out(api, direct, fs, pos, sps)
        assert cs.out_len(k) == want, (pos, k)
        o = cs.push(x[pos:pos + k])
        assert o.shape == (cs.n_sel, want), (pos, k, o.shape, want)
        outs.append(o)
        pos += k
    assert pos == x.size
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("schedule", ["one", "equal", "random"])
def test_filterbank_fast_path_streams_bit_identically(gpu_api, schedule):
    n = 600000 + 7
    x = _capture(n, FS, 11)
    ref = gpu_api.channelize(x, FS, CHANS)
    sizes = {"one": [n], "equal": [100000] * 6 + [7], "random": _random_sizes(n, 12)}[schedule]
    with gpu_api.ChanStream(FS, CHANS) as cs:
        got = _streamed(gpu_api, cs, x, sizes, FS)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)


def test_rotation_long_stream(gpu_api):
    """rotation != 0 over 20 s (40 M samples, past 2^24: 32-bit indices or float phases would show), 1 s pushes"""
    n = 40_000_000
    rng = np.random.default_rng(21)
    x = (rng.standard_normal((n, 2)) * 0.3).astype(np.float32).view(np.complex64).reshape(-1)
    x += np.exp(2j * np.pi * np.mod((5 * 31250.0 + 700.0) / FS * np.arange(n, dtype=np.float64), 1.0)).astype(np.complex64)
    chans = [4, 40, 63]
    rot = 2 * np.pi * 31250.0 / FS + 1e-4
    ref = gpu_api.channelize(x, FS, chans, rotation=rot)
    with gpu_api.ChanStream(FS, chans, rotation=rot) as cs:
        got = _streamed(gpu_api, cs, x, [2_000_000] * 20, FS)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("fs", [1.0e6, 1.25e6, 2.5e6, 4.0e6, 2.048e6, 1.92e6, 2.4e6])
def test_generic_filterbank_and_pre_resampler_stream_bit_identically(gpu_api, fs):
    """the generic filterbank (32, 40, 80, 128 channels) and, off the grid, the pre-resampler in front of it; with and
    without a rotation (off the grid the rotation is the pre-resampler's)"""
    M, _, _ = gpu_api.channelize_plan(fs, 4, 0)
    n = 40 * M * 50 + 37
    x = _capture(n, fs, int(fs) % 1000 + 5, M)
    chans = [3, M - 2, M // 2 - 1, 0, M - 1, M // 2]
    for rot in (0.0, 0.21):
        ref = gpu_api.channelize(x, fs, chans, rotation=rot)
        with gpu_api.ChanStream(fs, chans, rotation=rot) as cs:
            got = _streamed(gpu_api, cs, x, _random_sizes(n, int(fs) % 77, hi=n // 5), fs)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), (fs, rot)


@pytest.mark.parametrize("fs", [2.0e6, 1.25e6, 2.5e6, 4.0e6, 1.0e6])
def test_direct_mode_streams_bit_identically(gpu_api, fs):
    """the direct mode at the rates test_direct_mode_matches_oracle uses: d2 > 1, and 1.0 Msps with its 95-taps-per-phase
    resampler bank"""
    n = 200000 + 13
    x = _capture(n, fs, int(fs) % 97)
    freqs = [3 * 31250.0, -7 * 31250.0 + 400.0, 0.0]
    ref = gpu_api.ddc(x, fs, freqs)
    for sizes in ([n], _random_sizes(n, 3, hi=40000)):
        with gpu_api.ChanStream.direct(fs, freqs) as cs:
            got = _streamed(gpu_api, cs, x, sizes, fs, direct=True)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), fs


def test_counts_at_other_sps(gpu_api):
    """n_out(N + n) - n_out(N) per push at sps 1 and 2 (a longer input step per output), both modes"""
    n = 150000 + 3
    x = _capture(n, FS, 8)
    for sps in (1, 2):
        ref = gpu_api.channelize(x, FS, [5, 31], sps=sps)
        with gpu_api.ChanStream(FS, [5, 31], sps=sps) as cs:
            got = _streamed(gpu_api, cs, x, _random_sizes(n, sps, hi=20000), FS, sps=sps)
        assert np.array_equal(got, ref)
        d1, d2, rs, n_out = gpu_api.ddc_plan(FS, sps, n)
        ref = gpu_api.ddc(x, FS, [31250.0], sps=sps)
        with gpu_api.ChanStream.direct(FS, [31250.0], sps=sps) as cs:
            got = _streamed(gpu_api, cs, x, _random_sizes(n, sps + 7, hi=20000), FS, direct=True, sps=sps)
        assert np.array_equal(got, ref)


def _push_dev_run(api, cs, st, t, sizes, out, out_stride):
    import torch
    pos = done = 0
    with torch.cuda.stream(st):
        for k in sizes:
            w = cs.push_dev(st.cuda_stream, t.data_ptr() + 8 * pos, k, out.data_ptr() + 8 * done, out_stride)
            pos += k
            done += w
    return done


def test_device_resident_pushes_two_threads(gpu_api):
    """push_dev with torch device buffers on non-default streams: two handles pushed from two threads on two streams,
    interleaved; and one handle pushed alternately on two streams (each push waits for the one before)"""
    import torch
    n = 400000 + 5
    xs = [_capture(n, FS, 31), _capture(n, FS, 32)]
    chans = [[5, 40, 31], [0, 63, 12, 33]]
    refs = [gpu_api.channelize(xs[i], FS, chans[i]) for i in range(2)]
    n_out = refs[0].shape[1]
    ts = [torch.from_numpy(x.view(np.float32)).cuda() for x in xs]
    outs = [torch.zeros((len(c), n_out, 2), dtype=torch.float32, device="cuda") for c in chans]
    sts = [torch.cuda.Stream(), torch.cuda.Stream()]
    handles = [gpu_api.ChanStream(FS, c) for c in chans]
    done = [0, 0]
    errs = []

    def run(i):
        try:
            done[i] = _push_dev_run(gpu_api, handles[i], sts[i], ts[i], _random_sizes(n, 40 + i, hi=30000), outs[i], n_out)
        except Exception as e:       # surfaced below
            errs.append(e)

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for s in sts:
        s.synchronize()
    for i in range(2):
        assert done[i] == n_out
        got = outs[i].cpu().numpy().view(np.complex64).reshape(len(chans[i]), n_out)
        assert np.array_equal(got, refs[i]), i
        handles[i].close()
    # one handle, its pushes alternating between the two streams
    out = torch.zeros((3, n_out, 2), dtype=torch.float32, device="cuda")
    with gpu_api.ChanStream(FS, chans[0]) as cs:
        pos = dn = 0
        for j, k in enumerate(_random_sizes(n, 50, hi=30000)):
            st = sts[j % 2]
            with torch.cuda.stream(st):
                dn += cs.push_dev(st.cuda_stream, ts[0].data_ptr() + 8 * pos, k, out.data_ptr() + 8 * dn, n_out)
            pos += k
        torch.cuda.synchronize()
    assert dn == n_out
    assert np.array_equal(out.cpu().numpy().view(np.complex64).reshape(3, n_out), refs[0])


def test_refusals_leave_the_stream_as_it_was(gpu_api):
    with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
        gpu_api.ChanStream(FS, [5, 64])
    with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
        gpu_api.ChanStream(FS, [5, -1])
    with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
        gpu_api.ChanStream(FS, [5, 7, 5])
    with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
        gpu_api.ChanStream(1.9e6 + 0.5, [1])              # off the grid and not a whole number of Hz
    with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
        gpu_api.ChanStream.direct(23400.0 * 4 * 20, [0.0])  # an exact multiple of 23400 x sps: the reference cannot run it
    # plans whose resampler spans more than its window (csrc/chan_select.h) are refused when the handle is made, as the plan
    # and the one-shot call refuse them (test_direct_mode_refusals), not at the first push that has an output
    for fs in (1.0e6, 1.5e6):
        with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
            gpu_api.ChanStream.direct(fs, [0.0, 31250.0], sps=1)
        with gpu_api.ChanStream.direct(fs, [0.0, 31250.0], sps=2) as cs:
            assert cs.out_len(50000) == gpu_api.ddc_plan(fs, 2, 50000)[3]
    n = 200000 + 11
    x = _capture(n, FS, 41)
    ref = gpu_api.channelize(x, FS, [5, 40])
    lib = gpu_api.load()
    with gpu_api.ChanStream(FS, [5, 40]) as cs:
        a = cs.push(x[:70001])
        k = 50000
        need = cs.out_len(k)
        assert need > 0
        out = np.zeros((2, need), np.complex64)
        chunk = np.ascontiguousarray(x[70001:70001 + k])
        got = C.c_uint64(12345)
        rc = lib.gmr1_hip_chan_stream_push(cs._h, chunk.ctypes.data_as(C.c_void_p), C.c_uint64(k),
                                           out.ctypes.data_as(C.c_void_p), C.c_uint64(need - 1), C.byref(got))
        assert rc == -22
        rc = lib.gmr1_hip_chan_stream_push(cs._h, None, C.c_uint64(k), out.ctypes.data_as(C.c_void_p), C.c_uint64(need),
                                           C.byref(got))
        assert rc == -22
        assert cs.out_len(k) == need                       # nothing was counted
        b = cs.push(x[70001:])
    assert np.array_equal(np.concatenate([a, b], axis=1), ref)
