"""k_rx4 four bursts a wave (a wave asks for its four bursts' kind / offset together ahead of the first window, fetches each
window in one round trip and, in builds with GMR1_EXP_RX4_TOUCH, touches its next burst's window): the launch gives, bit for
bit, what the same bursts give as calls of at most 4096 -- those take the one-burst-a-wave path, which has no successor to
look at -- for batches whose last wave holds one, three, four and one
burst(s) behind a full one (n = 4097, 4099, 4100, 4101), in both decoder modes; and a strided sample agrees with the oracle.

The workload: BCCH and CCCH windows (1016 / 976 samples), the 1 : 6 mix in shuffled order, so that a burst's successor often
has the other length; no slack anywhere -- the first window starts at sample 0, every window starts where its
predecessor ends or (both lengths are multiples of 8 samples, so back to back alone only ever reaches two start residues)
one or two samples before that, which walks the starts through all 16 eight-byte residues of a 128-byte line; the last
window ends on the array's last sample.  The test provokes nothing and cannot see an out-of-range read: the addresses are
tests/test_rx4_touch_span.py's to check."""
import numpy as np
import pytest

import workloads

pytestmark = pytest.mark.gpu

N_MAX = 4101
KEYS = ("l2", "crc", "conv", "toa", "freq_err", "rv", "ebits", "ssyms")
_cache = {}


def _workload(pkg):
    if "wl" not in _cache:
        wl = workloads.bcch_ccch_mix(pkg, n=N_MAX, seed=58)
        perm = np.random.default_rng(58).permutation(N_MAX)          # BCCH and CCCH alternate irregularly
        src = wl["offset"][perm]
        wl["kind"], wl["l2"] = wl["kind"][perm], wl["l2"][perm]
        lens = np.where(wl["kind"] == 0, wl["in_len"][0], wl["in_len"][1]).astype(np.int64)
        back = np.arange(N_MAX) % 3                      # samples a window starts before its predecessor's end
        back[0] = 0
        start = np.zeros(N_MAX, np.int64)
        start[1:] = np.cumsum(lens[:-1] - back[1:])
        iq = np.zeros(int(start[-1] + lens[-1]), np.complex64)
        for i in range(N_MAX):
            a = int(src[i])
            iq[start[i]:start[i] + lens[i]] = wl["iq"][a:a + lens[i]]
        assert start[0] == 0 and len(set(int(s) % 16 for s in start)) == 16
        k = wl["kind"].astype(int)
        assert ((k[:-1] == 0) & (k[1:] == 1)).sum() > 100 and ((k[:-1] == 1) & (k[1:] == 0)).sum() > 100
        _cache["wl"] = dict(iq=iq, offset=start.astype(np.uint64), kind=wl["kind"], lens=lens, l2=wl["l2"])
    return _cache["wl"]


@pytest.mark.parametrize("n", [4097, 4099, 4100, 4101])
def test_four_a_wave_equals_one_a_wave_bit_for_bit(gpu_api, orc, pkg, decoder, n):
    wl = _workload(pkg)
    end = int(wl["offset"][n - 1]) + int(wl["lens"][n - 1])
    iq = wl["iq"][:end]                                  # the last window ends on the array's last sample
    off, kind = wl["offset"][:n], wl["kind"][:n]
    got = gpu_api.rx_bcch_ccch_batch(iq, off, kind, sps=4)
    parts = [gpu_api.rx_bcch_ccch_batch(iq, off[a:a + 4096], kind[a:a + 4096], sps=4) for a in range(0, n, 4096)]
    for k in KEYS:
        one = np.concatenate([p[k] for p in parts])
        assert got[k].shape == one.shape, k
        assert np.array_equal(got[k].view(np.uint8), one.view(np.uint8)), f"n {n}: {k} differs from the one-burst-a-wave calls"
    assert (got["crc"] == 0).mean() > 0.9
    good = got["crc"] == 0
    assert np.array_equal(got["l2"][good], wl["l2"][:n][good])
    # a strided sample against the oracle, the ends of the batch included (CRC verdicts and payloads, as test_gpu_rx.py)
    idx = np.unique(np.concatenate([np.arange(0, n, 53), np.arange(n - 6, n)]))
    key = (decoder, n)
    ref = orc.demod_decode_batch(iq, off[idx], kind[idx], sps=4, want_ebits=False, want_ssyms=False)
    assert np.array_equal(ref["crc"], got["crc"][idx]), key
    ok = ref["crc"] == 0
    assert np.array_equal(ref["l2"][ok], got["l2"][idx][ok]), key
