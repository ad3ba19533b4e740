"""GPU parity of the TCH3 follow-up pieces against the oracle: DKAB demodulator (reference
src/sdr/dkab.c), A5/1 keystream (reference src/l1/a5.c)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPS = 4


def _dkab_windows(pkg, n, seed, esn0_db=20.0, win=6, p_max=40, sps=SPS):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    rng = np.random.default_rng(seed)
    in_len = 117 * sps + win
    out = np.zeros((n, in_len), np.complex64)
    ps = rng.integers(0, p_max, n).astype(np.int32)
    bits = rng.integers(0, 2, size=(n, 8), dtype=np.uint8)
    present = rng.random(n) < 0.8
    sigma = np.sqrt(10.0 ** (-esn0_db / 10.0) / 2.0)
    for i in range(n):
        x = (rng.standard_normal((in_len + 40 * sps, 2)) * sigma).astype(np.float32).view(np.complex64).reshape(-1)
        if present[i]:
            body = synth.shape_bursts(synth.dkab_symbols(bits[i:i + 1], int(ps[i])), sps, float(rng.random()), 5)[0]
            x[:body.size] += body * np.exp(1j * rng.uniform(0, 2 * np.pi))
        d = int(rng.integers(0, win + 1))
        out[i] = x[5 * sps - d:5 * sps - d + in_len]
    return out, ps, bits, present


def test_dkab_demod_matches_oracle(gpu_api, orc, pkg):
    win, ps, bits, present = _dkab_windows(pkg, 300, 3)
    n, in_len = win.shape
    fs = np.random.default_rng(1).normal(0, 0.02, n).astype(np.float32)
    offset = np.arange(n, dtype=np.uint64) * np.uint64(in_len)
    rv, eb, toa = gpu_api.dkab_demod_batch(win.reshape(-1), offset, in_len, ps, sps=SPS, freq_shift=fs)
    n_found = 0
    bit_ok = bit_n = 0
    for i in range(n):
        orv, oeb, otoa = orc.dkab_demod(win[i], SPS, float(fs[i]), int(ps[i]))
        assert rv[i] == orv, (i, rv[i], orv)
        assert abs(toa[i] - otoa) < 2e-3, (i, toa[i], otoa)
        if orv == 0:
            n_found += 1
            assert np.max(np.abs(eb[i].astype(int) - oeb.astype(int))) <= 1, (i, eb[i], oeb)
            if present[i]:
                bit_ok += int(np.sum((eb[i] < 0).astype(np.uint8) == bits[i]))
                bit_n += 8
    assert n_found > 0.6 * n and np.all(rv[~present] == 1)
    assert bit_ok > 0.9 * bit_n, (bit_ok, bit_n)      # energy-only timing: the demodulator itself is coarse
    # the reference's own call
    r1, e1, t1 = gpu_api.dkab_demod(win[0], SPS, float(fs[0]), int(ps[0]))
    assert r1 == rv[0] and abs(t1 - toa[0]) < 1e-6 and (r1 or np.array_equal(e1, eb[0]))


def test_dkab_window_shorter_than_a_burst_is_an_error(gpu_api):
    x = np.zeros(100, np.complex64)
    with pytest.raises(Exception):
        gpu_api.dkab_demod_batch(x, [0], 100, 0, sps=SPS)


def test_a5_keystream_bit_exact(gpu_api, orc, pkg):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    rng = np.random.default_rng(9)
    n = 500
    keys = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)
    fn = rng.integers(0, 1 << 19, n).astype(np.uint32)
    fn[:4] = [0, 1, 0x7FFFF, 0xFFFFFFFF]
    dl, ul = gpu_api.a5_batch(1, keys, fn, 208, want_ul=True)
    for i in range(n):
        odl, oul = orc.a5(1, keys[i], int(fn[i]), 208)
        assert np.array_equal(dl[i], odl) and np.array_equal(ul[i], oul), i
    # a single bit and an odd length: the rows of the batch are nbits apart, whatever nbits is
    for nbits in (1, 77):
        dl2, ul2 = gpu_api.a5_batch(1, keys, fn, nbits, want_ul=True)
        assert dl2.shape == (n, nbits)
        for i in range(n):
            odl, oul = orc.a5(1, keys[i], int(fn[i]), nbits)
            assert np.array_equal(dl2[i], odl) and np.array_equal(ul2[i], oul), (nbits, i)
        assert np.array_equal(dl2, dl[:, :nbits])       # (the uplink block follows the downlink's nbits: no prefix of ul)
        d1, u1 = gpu_api.a5(1, keys[5], int(fn[5]), nbits)
        assert np.array_equal(d1, dl2[5]) and np.array_equal(u1, ul2[5])
    # second, independent implementation (numpy) over the whole batch
    k0 = keys[0]
    assert np.array_equal(gpu_api.a5_batch(1, k0, fn, 96), synth.a5_1(k0, fn.astype(np.int64) & 0xFFFFFFFF, 96))
    # A5/0 = zeros, unsupported algorithms leave the buffers alone (a5.c:56-78)
    assert not gpu_api.a5_batch(0, keys, fn, 64).any()
    d1, u1 = gpu_api.a5(1, keys[3], int(fn[3]), 208)
    assert np.array_equal(d1, dl[3]) and np.array_equal(u1, ul[3])
    d0, u0 = gpu_api.a5(0, keys[3], 5, 40)
    assert not d0.any() and not u0.any()
    d2, u2 = gpu_api.a5(2, keys[3], 5, 40)
    assert np.all(d2 == 0xEE) and np.all(u2 == 0xEE)
