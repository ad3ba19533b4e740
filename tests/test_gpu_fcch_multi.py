"""k_fcch_multi against the CPU oracle on the aimed windows of tests/fcch_multi_cases.py: lists that fill and overflow at
every size, duplicates one period apart and aliased ones, runs of threshold flags on every boundary of the kernel's flag
words, the strongest lag at either end of its range, other periods, the 468-symbol burst, windows without an answer.
tests/test_fcch_multi_host.py shows on the CPU that every window reaches what it is aimed at and that no float32 rounding
can decide any of them, so count and list are compared for equality."""
import numpy as np
import pytest

import acq_cases as ac
import fcch_multi_cases as fm

pytestmark = pytest.mark.gpu

CASES = fm.case_list()
FAR = np.complex64(1e6 - 1e6j)            # what lies between two windows: one sample of it in a sum and nothing agrees
SENTINEL = -777


def _groups():
    """the cases of one (type, sps, length, N) each: what one batch call takes"""
    g = {}
    for c in CASES:
        g.setdefault((c["which"], c["sps"], c["n"], c["N"]), []).append(c)
    return g


def _flat(pkg, cases, sps):
    """all windows in one array, at offsets that are no multiples of sps (nor even) -> (iq, offset, freq_shift)"""
    pos, offs = 1, []
    for c in cases:
        while pos % 2 == 0 or (sps > 1 and pos % sps == 0):
            pos += 1
        offs.append(pos)
        pos += c["n"] + 37
    iq = np.full(pos + 1024, FAR, np.complex64)
    for c, o in zip(cases, offs):
        iq[o:o + c["n"]] = fm.window(pkg, c)
    return iq, np.array(offs, np.uint64), np.array([c["fs"] for c in cases], np.float32)


@pytest.mark.parametrize("key", sorted(_groups()), ids=lambda k: "%s-sps%d-%d-N%d" % k)
def test_batch_entry_matches_the_oracle(gpu_api, orc, pkg, key):
    which, sps, n, N = key
    cases = _groups()[key]
    iq, off, fs = _flat(pkg, cases, sps)
    cnt, toa = gpu_api.fcch_rough_multi_batch(iq, off, n, sps=sps, freq_shift=fs, N=N, fcch_type=which)
    for i, c in enumerate(cases):
        want = fm.expected(pkg, orc, c)
        got = (int(cnt[i]), [int(t) for t in toa[i, :max(int(cnt[i]), 0)]])
        assert got == want, (c["name"], got, want)
        assert not toa[i, max(want[0], 0):].any(), (c["name"], toa[i])          # the host form hands back zeros there


def test_reference_single_call(gpu_api, orc, pkg):
    """gmr1_fcch_rough_multi itself on the first case of every group; N outside 1..32 is refused"""
    for key, cases in sorted(_groups().items()):
        c = cases[0]
        rv, toa = gpu_api.fcch_rough_multi(fm.window(pkg, c), c["sps"], c["fs"], c["N"], c["which"])
        assert (rv, [int(t) for t in toa]) == fm.expected(pkg, orc, c), c["name"]
    x = fm.window(pkg, CASES[0])
    for N in (0, 33):
        assert gpu_api.fcch_rough_multi(x, CASES[0]["sps"], 0.0, N)[0] == -22


def test_device_entry_leaves_the_rest_of_a_row_alone(gpu_api, orc, pkg):
    """gmr1_hip_fcch_rough_multi_batch_dev over rows that held something else: entries [count, N) of a row still hold it
    (k_fcch_multi: "the caller's array beyond stays as it was"), and so does the whole row of a stream that answers -22"""
    import torch
    key = ("fcch", 4, fm.min_len(4), 16)                  # the shortest windows: the two without an answer are among them
    cases = _groups()[key]
    assert {"zeros", "constant"} <= {c["name"] for c in cases}
    which, sps, n, N = key
    iq, off, fs = _flat(pkg, cases, sps)
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_fs = torch.from_numpy(fs).cuda()
    d_toa = torch.full((len(cases), N), SENTINEL, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((len(cases),), SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()                             # the copies and fills above ran on another stream than the call
    gpu_api._call("gmr1_hip_fcch_rough_multi_batch_dev", st.cuda_stream, gpu_api._fcch_id(which), len(cases), sps, n,
                  d_iq.data_ptr(), d_off.data_ptr(), d_fs.data_ptr(), d_toa.data_ptr(), N, d_cnt.data_ptr())
    st.synchronize()
    cnt, toa = d_cnt.cpu().numpy(), d_toa.cpu().numpy()
    for i, c in enumerate(cases):
        want = fm.expected(pkg, orc, c)
        k = max(want[0], 0)
        assert int(cnt[i]) == want[0] and [int(t) for t in toa[i, :k]] == want[1], (c["name"], cnt[i], toa[i], want)
        assert (toa[i, k:] == SENTINEL).all(), (c["name"], toa[i])
    assert sum(int(v) == -22 for v in cnt) >= 2 and any(0 < int(v) < N for v in cnt)


def test_acquisition_with_a_full_and_an_aliased_list(gpu_api, orc, pkg):
    """gmr1_hip_fcch_acquire_batch on a carrier whose step 3 gets a full list of sixteen candidates and on one with an
    aliased duplicate: the records of acq_cases.expected, under its MARGIN rule"""
    cases = fm.acq_carriers(pkg)
    want = ac.expected_all(orc, cases)
    assert want[0]["n_cand"] == ac.MAX_CHAINS and want[1]["n_cand"] == 2
    iq, off, ln = ac.pack([x for _, x, _ in cases])
    got = gpu_api.fcch_acquire(iq, off, ln, start=[s for _, _, s in cases])
    for (name, _, _), g, w in zip(cases, got, want):
        ac.check_record(name, g, w)


def test_constant_window_is_a_zero_window_to_the_rough_sweep(gpu_api):
    """A window without deviation is all zero once normalised, so every lag's energy is 0 -- in the small launch
    (k_fcch_energy applies the statistics) and in a launch large enough to be folded (k_fcch_sweep does): the single-peak
    rough entry answers a constant window exactly as it answers an all-zero one.  That answer is rv 0, toa 0: the
    reference's is (int)round(0 / 0), undefined in C, and the acquisition chain adds this toa to a window's offset."""
    n = 30888
    pair = np.stack([np.zeros(n, np.complex64), np.full(n, 0.5 - 0.25j, np.complex64)])
    for copies in (1, 80):                               # 2 and 160 streams of 4 lag tiles: 8 and 640 work-groups
        x = np.tile(pair, (copies, 1))
        toa, rv = gpu_api.fcch_rough_batch(x, (np.arange(2 * copies) * n).astype(np.uint64), n, sps=4)
        assert list(toa[0::2]) == list(toa[1::2]) and list(rv[0::2]) == list(rv[1::2])
        assert not toa.any() and not rv.any(), (toa[:2], rv[:2])
