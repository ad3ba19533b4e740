"""GPU tests of the streaming receive loop (gmr1_hip_rx_stream_*): any sequence of pushes gives, once sorted by
(carrier, chain), byte for byte the records of one gmr1_hip_rx_run call on the same samples, and its status / n_chains."""
import ctypes as C
import threading

import numpy as np
import pytest

import workloads

pytestmark = pytest.mark.gpu

SPS = 4
FRAME = 24 * 39 * SPS
H_ACQ = 8000 + 330 * 234 * SPS // 10 + 650 * 234 * SPS // 10 + 3 * 117 * SPS     # rx_stream.h: rx_stream_acq_need
SINGLES = 2 * FRAME + 500                  # the "singles" schedule's run of one-sample pushes past 1.5 s


def _carriers(pkg, seconds=3.0):
    """carriers of mixed timeslot, SI1 delay, CFO and SNR (test_gpu_rxloop's mix), two transmitters on one, one of noise"""
    specs = [
        dict(seed=11, stn=3, delay=2, cfo_hz=120.0, esn0_db=15.0),
        dict(seed=12, stn=0, delay=0, cfo_hz=-300.0, esn0_db=12.0),
        dict(seed=13, stn=17, delay=5, cfo_hz=0.0, esn0_db=20.0),
        dict(seed=14, stn=9, delay=7, cfo_hz=250.0, esn0_db=9.0),
        dict(seed=15, stn=21, delay=1, cfo_hz=-80.0, esn0_db=7.0, p_idle=0.5),
    ]
    out = []
    for sp in specs:
        sp = dict(sp)
        x, _ = workloads.bcch_carrier(pkg, sp.pop("seed"), seconds=seconds, sps=SPS, **sp)
        out.append(x)
    a, _ = workloads.bcch_carrier(pkg, 21, seconds=seconds, sps=SPS, stn=2, delay=3, cfo_hz=60.0, esn0_db=18.0, t0=1000)
    b, _ = workloads.bcch_carrier(pkg, 22, seconds=seconds, sps=SPS, stn=2, delay=3, cfo_hz=90.0, esn0_db=18.0,
                                  t0=1000 + 11 * 39 * SPS)
    out.append((a + 0.8 * b).astype(np.complex64))
    n = min(x.size for x in out)
    rng = np.random.default_rng(99)
    out.append(rng.standard_normal((n, 2), dtype=np.float32).view(np.complex64).reshape(-1))
    return np.stack([x[:n] for x in out]).astype(np.complex64)


def _one_shot(api, x, arfcn):
    A, n = x.shape
    offset = np.arange(A, dtype=np.uint64) * np.uint64(n)
    length = np.full(A, n, np.uint64)
    rec, status, chains, found = api.rx_run(x.reshape(-1), offset, length, sps=SPS, arfcn=arfcn, max_records=1 << 20)
    assert found == len(rec)
    return rec, status, chains


def _sorted(rec, arfcn):
    """stable sort by (carrier, chain)"""
    pos = {int(a): i for i, a in enumerate(arfcn)}
    key = np.array([pos[int(a)] * 256 + int(c) for a, c in zip(rec["arfcn"], rec["chain"])], np.int64)
    return rec[np.argsort(key, kind="stable")] if len(rec) else rec


def _stream(api, x, sizes, arfcn, last_empty=False):
    """push x in pieces of the given sizes (the rest in the last one) -> (records, status, n_chains, per-push counts)"""
    A, n = x.shape
    got, at, counts = [], 0, []
    with api.RxStream(A, sps=SPS, arfcn=arfcn) as s:
        for k in sizes:
            k = min(int(k), n - at)
            if at + k >= n and not last_empty:
                break
            r = s.push(x[:, at:at + k])
            got.append(r.copy())
            counts.append(len(r))
            at += k
        if last_empty:
            got.append(s.push(x[:, at:]).copy())
            got.append(s.push(np.zeros((A, 0), np.complex64), last=True).copy())
        else:
            got.append(s.push(x[:, at:], last=True).copy())
        status, chains, _ = s.status()
    rec = np.concatenate(got) if got else np.empty(0, api.RX_RECORD)
    return rec, status, chains, counts


def _check_same(api, x, arfcn, rec, status, chains):
    ref, rst, rch = _one_shot(api, x, arfcn)
    assert np.array_equal(status, rst[:len(status)]), (status, rst)
    assert np.array_equal(chains, rch[:len(chains)]), (chains, rch)
    mine = _sorted(rec, arfcn)
    assert len(mine) == len(ref), (len(mine), len(ref))
    assert mine.tobytes() == ref.tobytes(), "streamed records differ from the one-shot call's"
    return ref


def _schedule(name, n):
    rng = np.random.default_rng(7)
    if name == "one":
        return []
    if name == "10ms":
        return [936] * (n // 936 + 1)
    if name == "random":
        s = []
        while sum(s) < n:
            s.append(int(rng.choice([0, 1, 7, 100, 936, 3001, 20000, 90000])))
        return s
    if name == "singles":
        # big pushes up to H_acq - 40, single samples over H_acq, one chunk to 1.5 s, then single samples over more than
        # two frame lengths: every chain's release point (align + 2 * frame_len) passes inside them at least twice
        s = [H_ACQ - 40] + [1] * 80
        s += [140400 - sum(s) - 200] + [1] * SINGLES
        s += [50000] * (n // 50000 + 1)
        return s
    raise ValueError(name)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("sched", ["one", "10ms", "random", "singles", "last0"])
def test_stream_matches_one_shot(gpu_api, pkg, decoder, sched):
    x = _carriers(pkg)
    arfcn = np.arange(x.shape[0], dtype=np.uint16) + 200
    sizes = _schedule("10ms" if sched == "last0" else sched, x.shape[1])
    rec, status, chains, counts = _stream(gpu_api, x, sizes, arfcn, last_empty=sched == "last0")
    ref = _check_same(gpu_api, x, arfcn, rec, status, chains)
    assert len(ref) > 200 and (chains > 1).any()
    if sched != "one":
        assert sum(c > 0 for c in counts) >= 2, "records should come out before the end of the capture"
    if sched == "singles":
        # chains were released and walked a frame inside the one-sample pushes: each of those frames came out there
        run = counts[82:82 + SINGLES]
        assert sum(c > 0 for c in run) >= 8, sum(c > 0 for c in run)


@pytest.mark.timeout(300)
def test_stream_matches_oracle_per_carrier(gpu_api, orc, pkg):
    x = _carriers(pkg, seconds=2.5)
    arfcn = np.arange(x.shape[0], dtype=np.uint16) + 10
    rec, status, chains, _ = _stream(gpu_api, x, [20000] * 100, arfcn)
    for i in range(x.shape[0]):
        orv, orec, och = orc.rx_run(x[i], sps=SPS, arfcn=int(arfcn[i]))
        mine = rec[rec["arfcn"] == arfcn[i]]
        mine = mine[np.argsort(mine["chain"], kind="stable")] if len(mine) else mine
        assert (status[i] == 0) == (orv == 0), (i, status[i], orv)
        if orv:
            assert len(mine) == 0
            continue
        assert chains[i] == och
        keys = lambda r: [(int(q["chain"]), int(q["type"]), int(q["fn"]), int(q["tn"]), bytes(q["l2"])) for q in r]
        assert keys(mine) == keys(orec), f"carrier {i}"


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [20000, H_ACQ - 1, H_ACQ, H_ACQ + 1, H_ACQ + FRAME])
def test_stream_capture_ends_near_acquisition(gpu_api, pkg, n):
    x = _carriers(pkg, seconds=1.5)[:, :n]
    arfcn = np.arange(x.shape[0], dtype=np.uint16)
    for sizes in ([], [H_ACQ - 3, 1, 1, 1, 1], [5000] * 30):
        rec, status, chains, _ = _stream(gpu_api, np.ascontiguousarray(x), sizes, arfcn)
        _check_same(gpu_api, np.ascontiguousarray(x), arfcn, rec, status, chains)


@pytest.mark.timeout(300)
def test_stream_si1_moves_timeslot_31_to_0(gpu_api, pkg):
    """an SI1 that relabels stn 31 as 0 (align jumps by 1209 sps) and back, right after push boundaries"""
    streams = []
    for seed, lie in ((501, {6: (2, 0)}), (502, {5: (2, 0), 9: (2, 31)})):
        s, _ = workloads.bcch_carrier(pkg, seed, seconds=3.0, sps=SPS, stn=31, delay=2, cfo_hz=40.0, esn0_db=18.0,
                                      si1_lie=lie)
        streams.append(s)
    n = min(s.size for s in streams)
    x = np.stack([s[:n] for s in streams]).astype(np.complex64)
    arfcn = np.array([7, 8], np.uint16)
    for step in (311, 936, 1500):
        rec, status, chains, _ = _stream(gpu_api, x, [step] * (n // step + 1), arfcn)
        _check_same(gpu_api, x, arfcn, rec, status, chains)


def _mis_speculation_carriers(pkg, seconds=6.0):
    """carriers on which the loop's speculative front is wrong again and again: CRC failures, missing bursts, a late
    first SI1, SI1s that relabel timeslot or frame count, strong noise bursts"""
    specs = [
        dict(seed=301, stn=4, delay=1, cfo_hz=70.0, esn0_db=4.0),
        dict(seed=303, stn=11, delay=6, cfo_hz=30.0, esn0_db=14.0, absent_bcch=range(2, 36, 3)),
        dict(seed=304, stn=19, delay=2, cfo_hz=200.0, esn0_db=14.0, other_first=8),
        dict(seed=305, stn=5, delay=4, cfo_hz=-40.0, esn0_db=16.0, si1_lie={6: (4, 9), 7: (4, 9)}),
        dict(seed=306, stn=2, delay=0, cfo_hz=10.0, esn0_db=16.0, si1_lie={5: (3, 2)}),
    ]
    out = []
    for sp in specs:
        sp = dict(sp)
        x, _ = workloads.bcch_carrier(pkg, sp.pop("seed"), seconds=seconds, sps=SPS, **sp)
        out.append(x)
    rng = np.random.default_rng(5)
    x = out[0].copy()
    for pos in rng.integers(0, x.size - 6000, 12):
        x[pos:pos + 5000] = rng.standard_normal((5000, 2), dtype=np.float32).view(np.complex64).reshape(-1) * np.float32(3.0)
    out.append(x)
    n = min(s.size for s in out)
    return np.stack([s[:n] for s in out]).astype(np.complex64)


@pytest.mark.timeout(600)
def test_stream_forced_mis_speculation(gpu_api, pkg, decoder):
    x = _mis_speculation_carriers(pkg)
    arfcn = np.arange(x.shape[0], dtype=np.uint16) + 40
    for sizes in ([9360] * 60, list(np.random.default_rng(3).integers(0, 30000, 80))):
        rec, status, chains, _ = _stream(gpu_api, x, sizes, arfcn)
        _check_same(gpu_api, x, arfcn, rec, status, chains)


@pytest.mark.timeout(900)
def test_stream_64_carriers_20_s_bounded(gpu_api, pkg):
    seconds, push = 20.0, 93600
    base = []
    for k in range(8):
        x, _ = workloads.bcch_carrier(pkg, 700 + k, seconds=seconds, sps=SPS, stn=(5 * k) % 32, delay=k % 8,
                                      cfo_hz=30.0 * k - 100.0, esn0_db=12.0 + k)
        base.append(x)
    n = min(x.size for x in base)
    x = np.stack([base[i % 8][:n] for i in range(64)]).astype(np.complex64)
    arfcn = np.arange(64, dtype=np.uint16) + 300
    got = []
    with gpu_api.RxStream(64, sps=SPS, arfcn=arfcn) as s:
        at = 0
        while at < n:
            k = min(push, n - at)
            got.append(s.push(x[:, at:at + k], last=at + k >= n).copy())
            at += k
            status, chains, retained = s.status()
            if at >= H_ACQ and at < n:
                live = (status == 0) & (chains > 0)
                assert live.sum() >= 60
                assert (retained[live] <= push + 4 * FRAME + 64).all(), retained.max()
                assert (retained[~live] == 0).all()
        status, chains, retained = s.status()
        assert (retained == 0).all()
    rec = np.concatenate(got)
    _check_same(gpu_api, x, arfcn, rec, status, chains)


@pytest.mark.timeout(600)
def test_stream_device_pipeline_from_channelizer(gpu_api, pkg):
    import torch
    FS = 2.0e6
    carriers = ((3, dict(stn=3, delay=2, cfo_hz=80.0)), (17, dict(stn=10, delay=5, cfo_hz=-150.0)),
                (60, dict(stn=0, delay=0, cfo_hz=20.0)))
    wide, _ = workloads.wideband_capture(pkg, 11, seconds=2.5, carriers=carriers)
    chans = [c for c, _ in carriers] + [30]
    nb = gpu_api.channelize(wide, FS, chans)
    arfcn = np.asarray(chans, np.uint16)
    ref, rst, rch = _one_shot(gpu_api, np.ascontiguousarray(nb), arfcn)
    w = torch.from_numpy(wide.view(np.float32)).cuda()
    rng = np.random.default_rng(17)
    torch_stream = torch.cuda.Stream()
    st = torch_stream.cuda_stream
    got = []
    cs = gpu_api.ChanStream(FS, chans)
    rs = gpu_api.RxStream(len(chans), sps=4, arfcn=arfcn)
    try:
        at = 0
        while at < wide.size:
            k = int(min(rng.choice([0, 1000, 37000, 200000]), wide.size - at))
            last = at + k >= wide.size
            n_out = cs.out_len(k)
            out = torch.empty((len(chans), max(n_out, 1) * 2), dtype=torch.float32, device="cuda")
            with torch.cuda.stream(torch_stream):
                got_n = cs.push_dev(st, w.data_ptr() + 8 * at, k, out.data_ptr(), max(n_out, 1))
                assert got_n == n_out
                got.append(rs.push_dev(st, out.data_ptr(), max(n_out, 1), n_out, last=last).copy())
            at += k
        status, chains, _ = rs.status()
    finally:
        cs.close()
        rs.close()
    mine = _sorted(np.concatenate(got), arfcn)
    assert np.array_equal(status, rst) and np.array_equal(chains, rch)
    assert mine.tobytes() == ref.tobytes()
    assert len(ref) > 100


@pytest.mark.timeout(300)
def test_stream_refusals_leave_the_handle_unchanged(gpu_api, pkg):
    x = _carriers(pkg, seconds=2.0)[:2]
    x = np.ascontiguousarray(x)
    arfcn = np.array([1, 2], np.uint16)
    with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
        gpu_api.RxStream(2, sps=17)
    with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
        gpu_api.RxStream(0, sps=4)
    ref, rst, rch = _one_shot(gpu_api, x, arfcn)
    with gpu_api.RxStream(2, sps=SPS, arfcn=arfcn) as s:
        got, at = [], 0
        for k in (50000, 70000, 30000):
            m = s.max_records(k)
            if m > 0:
                small = np.empty(m - 1 if m > 1 else 1, gpu_api.RX_RECORD)
                if m > 1:
                    with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
                        s.push(x[:, at:at + k], out=small)
            got.append(s.push(x[:, at:at + k]).copy())
            at += k
        got.append(s.push(x[:, at:], last=True).copy())
        with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
            s.push(x[:, :10])
        status, chains, _ = s.status()
    mine = _sorted(np.concatenate(got), arfcn)
    assert np.array_equal(status, rst) and np.array_equal(chains, rch)
    assert mine.tobytes() == ref.tobytes()


@pytest.mark.timeout(600)
def test_stream_two_handles_two_threads(gpu_api, pkg):
    import torch
    xa = _carriers(pkg, seconds=2.5)
    xb = np.ascontiguousarray(xa[::-1])
    arfcn = np.arange(xa.shape[0], dtype=np.uint16)
    solo = [_stream(gpu_api, x, [7000] * 60, arfcn)[0] for x in (xa, xb)]
    res = [None, None]
    errs = []

    def run(i, x):
        try:
            s_t = torch.cuda.Stream()
            d = torch.from_numpy(x.view(np.float32).reshape(x.shape[0], -1)).cuda()
            torch.cuda.synchronize()
            got, at, n = [], 0, x.shape[1]
            with gpu_api.RxStream(x.shape[0], sps=SPS, arfcn=arfcn) as s:
                while at < n:
                    k = min(7000, n - at)
                    got.append(s.push_dev(s_t.cuda_stream, d.data_ptr() + 8 * at, n, k, last=at + k >= n).copy())
                    at += k
            res[i] = np.concatenate(got)
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(i, x)) for i, x in enumerate((xa, xb))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert res[i].tobytes() == solo[i].tobytes()


@pytest.mark.timeout(120)
def test_stream_push_from_another_device_is_refused(gpu_api, pkg):
    """a handle belongs to the device it was created on: a push from a thread on another device is refused, and the
    handle then works as if it had not been tried"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    x = _carriers(pkg, seconds=1.5)[:2]
    x = np.ascontiguousarray(x)
    arfcn = np.array([1, 2], np.uint16)
    ref, rst, rch = _one_shot(gpu_api, x, arfcn)
    err = []
    with gpu_api.RxStream(2, sps=SPS, arfcn=arfcn) as s:
        def other():
            try:
                gpu_api.init(1)
                with pytest.raises(gpu_api.Gmr1HipError, match="-22"):
                    s.push(x[:, :1000])
            except BaseException as e:        # noqa: BLE001
                err.append(e)
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert not err, err
        rec = s.push(x, last=True)
        status, chains, _ = s.status()
    assert np.array_equal(status, rst) and np.array_equal(chains, rch)
    assert _sorted(rec, arfcn).tobytes() == ref.tobytes()


@pytest.mark.timeout(60)
def test_each_kind_of_handle_takes_its_own_push_entry_and_no_other(gpu_api):
    """The four kinds of handle against the four device push entries, no samples moved (n = 0, not the last push): the
    twelve wrong pairings are refused with every count zeroed and a message that names the handle's maker, its entry and
    the entry tried; the right pairing, made after them on the same handle, goes through with nothing found, and the
    handle then holds nothing and reports no error."""
    api = gpu_api
    kinds = {"": {}, "_tch": dict(tch=True), "_full": dict(full=True), "_voice": dict(voice=True)}
    last_error = api._fn("gmr1_hip_last_error")
    for mine, flags in kinds.items():
        with api.RxStream(1, sps=SPS, **flags) as s:
            out = np.empty(max(s.max_records(0), 1), api.RX_RECORD)
            big = np.empty(max(s.max_big(0), 1), api.RX_BIG_RECORD)
            audio = np.empty(max(s.max_audio(0), 1), api.RX_AUDIO)
            assert out.size > 1 and (big.size > 1) == (mine == "_full") and (audio.size > 1) == (mine == "_voice")

            def push(tried):
                """the device entry `tried` on this handle -> (return code, the counts it was given)"""
                counts = [C.c_int(7)]
                chunks = {"": (None,), "_tch": (None, None), "_full": (None, None, None), "_voice": (None, None)}[tried]
                tail = ()
                if tried in ("_full", "_voice"):
                    extra = big if tried == "_full" else audio
                    counts.append(C.c_int(7))
                    tail = (extra.ctypes.data, extra.size, C.byref(counts[1]))
                rc = api._fn("gmr1_hip_rx_stream_push%s_dev" % tried)(None, s._h, *chunks, 0, 0, 0, out.ctypes.data, out.size,
                                                                      C.byref(counts[0]), *tail)
                return rc, [c.value for c in counts]

            for tried in kinds:
                if tried == mine:
                    continue
                rc, counts = push(tried)
                assert rc == -22 and not any(counts), (mine, tried, rc, counts)
                want = "a handle of gmr1_hip_rx_stream_create%s takes gmr1_hip_rx_stream_push%s*, not gmr1_hip_rx_stream_push%s*" % (
                    mine, mine, tried)
                assert want.encode() in last_error(), (mine, tried, last_error())
            rc, counts = push(mine)
            assert rc == 0 and not any(counts), (mine, rc, counts, last_error())
            status, chains, retained = s.status()
            assert not status.any() and not chains.any() and not retained.any(), (mine, status, chains, retained)
