"""GPU tests of the batched FCCH acquisition (gmr1_hip_fcch_acquire_batch*): one record per stream, equal to what the CPU
oracle's FCCH primitives give when they are run in gmr1_rx's order (tests/acq_cases.py), the decisions included."""
import threading

import numpy as np
import pytest

import acq_cases as ac

pytestmark = pytest.mark.gpu

_check, _expect = ac.check_record, ac.expected_all


@pytest.fixture(scope="module")
def plain(pkg, orc):
    """the call with start = NULL (tests/acq_cases.py: plain_streams) and what it has to give"""
    cases = [(name, x, 8000) for name, x in ac.plain_streams(pkg)]
    iq, off, ln = ac.pack([x for _, x, _ in cases])
    return dict(cases=cases, iq=iq, off=off, ln=ln, want=_expect(orc, cases))


def test_plain_streams_match_the_oracle(gpu_api, plain):
    """Six carriers, noise, a stream without the 330 ms window and one without the 650 ms window, in one call of the host
    form (which, knowing the lengths, runs rough_multi over the long ones only)."""
    got = gpu_api.fcch_acquire(plain["iq"], plain["off"], plain["ln"])
    for (name, _, _), g, w in zip(plain["cases"], got, plain["want"]):
        _check(name, g, w)
    by = {name: w for (name, _, _), w in zip(plain["cases"], plain["want"])}
    assert all(by["carrier%d" % i]["status"] == 0 and by["carrier%d" % i]["n_chains"] >= 1 for i in range(6))
    assert by["carrier5"]["n_cand"] > by["carrier5"]["n_chains"]           # candidates dropped for their SNR
    assert by["short"]["status"] == -1 and by["no650"]["status"] == -1


def test_pairs_and_start_match_the_oracle(gpu_api, orc, pkg):
    """Two carriers on top of each other -- a second chain, a candidate dropped for its frequency -- and a start of its own."""
    cases = [(name, x, start) for name, x, start in ac.pair_streams(pkg)]
    want = _expect(orc, cases)
    iq, off, ln = ac.pack([x for _, x, _ in cases])
    got = gpu_api.fcch_acquire(iq, off, ln, start=[s for _, _, s in cases])
    for (name, _, _), g, w in zip(cases, got, want):
        _check(name, g, w)
    by = {name: w for (name, _, _), w in zip(cases, want)}
    assert by["pair_0.6_+100Hz"]["n_chains"] == 2
    assert by["pair_0.6_+800Hz"]["n_cand"] == 2 and by["pair_0.6_+800Hz"]["n_chains"] == 1
    assert by["late_start"]["align"] >= 23456


def test_fcch3_and_other_sample_rates(gpu_api, orc, pkg):
    """The 468-symbol chirp (fcch_type 1), and a carrier at 1 and at 16 samples per symbol."""
    x = ac.fcch3_stream(pkg)
    want = _expect(orc, [("fcch3", x, 8000)], which="fcch3_lband")[0]
    assert want["status"] == 0 and want["n_chains"] == 1
    _check("fcch3", gpu_api.fcch_acquire(x, [0], [x.size], fcch_type="fcch3_lband")[0], want)
    for sps, seed in ((1, 531), (16, 532)):
        x = ac.carrier(pkg, seed, sps=sps)
        want = _expect(orc, [("sps%d" % sps, x, 8000)], sps=sps)[0]
        assert want["status"] == 0 and want["n_chains"] >= 1
        _check("sps%d" % sps, gpu_api.fcch_acquire(x, [0], [x.size], sps=sps)[0], want)


def test_receive_loop_follows_the_same_chains(gpu_api, plain):
    """gmr1_hip_rx_run reads its acquisition from the same records: status and chains per carrier are the new call's"""
    keep = [i for i, (name, _, _) in enumerate(plain["cases"]) if name != "noise"]
    got = gpu_api.fcch_acquire(plain["iq"], plain["off"][keep], plain["ln"][keep])
    _, status, chains, _ = gpu_api.rx_run(plain["iq"], plain["off"][keep], plain["ln"][keep], sps=ac.SPS)
    assert list(status) == list(got["status"]) and list(chains) == list(got["n_chains"])
    assert list(status) == [0] * 6 + [-1, -1]


def _dev_call(api, torch, stream, d_iq, off, ln):
    """the _dev entry over device tensors -> the records, as bytes came back"""
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_len = torch.from_numpy(ln.astype(np.int64)).cuda()
    d_out = torch.full((off.size * api.FCCH_ACQ.itemsize,), 0xa5, dtype=torch.uint8, device="cuda")
    api.fcch_acquire_dev(stream.cuda_stream, off.size, d_iq.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_out.data_ptr(),
                         sps=ac.SPS)
    stream.synchronize()
    return d_out.cpu().numpy().tobytes()


def test_device_form_returns_the_host_forms_bytes(gpu_api, plain):
    """Everything in device memory (the lengths too: rough_multi then runs over every slot, the short streams' on the spare
    window): the same bytes as the host form, over records that held something else before."""
    import torch
    host = gpu_api.fcch_acquire(plain["iq"], plain["off"], plain["ln"]).tobytes()
    d_iq = torch.from_numpy(plain["iq"].view(np.float32)).cuda()
    assert _dev_call(gpu_api, torch, torch.cuda.Stream(), d_iq, plain["off"], plain["ln"]) == host


def test_two_threads_get_what_one_call_gets(gpu_api, plain):
    """Two threads, a stream each, different streams of the batch, several times over: each gets its rows of the single call"""
    import torch
    size = gpu_api.FCCH_ACQ.itemsize
    host = gpu_api.fcch_acquire(plain["iq"], plain["off"], plain["ln"]).tobytes()
    d_iq = torch.from_numpy(plain["iq"].view(np.float32)).cuda()
    n = plain["off"].size
    parts = [np.arange(0, n // 2), np.arange(n // 2, n)]
    errs, done = [], []
    go = threading.Barrier(2)

    def work(rows):
        try:
            st = torch.cuda.Stream()
            go.wait()
            for it in range(3):
                got = _dev_call(gpu_api, torch, st, d_iq, plain["off"][rows], plain["ln"][rows])
                assert got == host[rows[0] * size:(rows[-1] + 1) * size], f"iteration {it}"
            done.append(True)
        except BaseException as e:      # noqa: BLE001 - reported by the main thread
            errs.append(repr(e))

    ts = [threading.Thread(target=work, args=(rows,)) for rows in parts]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    assert len(done) == 2
