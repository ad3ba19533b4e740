"""GPU tests of the streaming receive loop with the TCH3 follow-up (gmr1_hip_rx_stream_create_tch / _push_tch*): any
sequence of pushes gives, once sorted by (carrier, chain), byte for byte the records of one gmr1_hip_rx_run_tch call on
the same samples with the same keys, and its status / n_chains; and of gmr1_hip_tch3_state_assign_batch_dev, rx_tch3_init
on states that stay in device memory."""
import ctypes as C

import numpy as np
import pytest

import rx_stream_tch_cases as cases
import tch3_cases as tc
import test_gpu_rx_stream as plain

pytestmark = pytest.mark.gpu

SPS = cases.SPS
FRAME = 24 * 39 * SPS


def _is_imm_ass(r):
    return r["type"] == 2 and r["l2"][1] == 0x06 and r["l2"][2] == 0x3f


def _check_same(api, name, cap, arfcn, rec, status, chains):
    ref, rst, rch = cases.one_shot(api, name, cap, arfcn)
    assert np.array_equal(status, rst), (status, rst)
    assert np.array_equal(chains, rch), (chains, rch)
    mine = plain._sorted(rec, arfcn)
    assert len(mine) == len(ref), (len(mine), len(ref))
    assert mine.tobytes() == ref.tobytes(), "streamed records differ from the one-shot call's"
    return ref


@pytest.mark.timeout(600)
@pytest.mark.parametrize("sched", ["one", "10ms", "random", "singles"])
def test_stream_tch_matches_one_shot(gpu_api, pkg, decoder, sched):
    """Four carriers with a call each (plain, ciphered after 30 frames, ciphered from the start, ending) and one whose
    traffic side is noise, all 4.0 s: that length gives every seed what the input condition below asks for."""
    cap = cases.pairs(pkg)
    arfcn = np.arange(cap["x"].shape[0], dtype=np.uint16) + 200
    # the input, judged on the one-shot result: enough traffic records, and ciphering switched on where there is a key
    ref, _, _ = cases.one_shot(gpu_api, "pairs", cap, arfcn)
    assert int(np.sum(ref["type"] >= 0x10)) >= 100
    for i, msgs in cap["ciphered"].items():
        mine = ref[(ref["arfcn"] == arfcn[i]) & (ref["type"] == 0x12)]
        assert any(bytes(r["l2"][:10]) in msgs for r in mine), f"carrier {i}: no deciphered FACCH3 message"
    rec, status, chains, pushes = cases.stream(gpu_api, cap["x"], cap["t"], cap["kc"], plain._schedule(sched, cap["x"].shape[1]), arfcn)
    _check_same(gpu_api, "pairs", cap, arfcn, rec, status, chains)
    if sched != "one":
        assert sum(bool((p["type"] >= 0x10).any()) for p in pushes) >= 2, "traffic records should come out as the call goes on"
    for p in pushes:
        # within a push: by carrier, chain; a frame's BCCH / CCCH records before its TCH3 record is part of the identity above
        key = p["arfcn"].astype(np.int64) * 256 + p["chain"]
        assert (np.diff(key) >= 0).all()


@pytest.mark.timeout(600)
def test_stream_tch_reassignments(gpu_api, pkg, decoder):
    """Several IMMEDIATE ASSIGNMENTs on one chain: in one push (several invocations of the follower, an assignment on the
    device before each) and at 10 ms (each assignment in a push of its own, the call before it carried in)."""
    cap = cases.reassigned(pkg)
    arfcn = np.array([0, 1], np.uint16)
    ref, _, _ = cases.one_shot(gpu_api, "reassigned", cap, arfcn)
    for i, ia in enumerate(cap["ia"]):
        mine = ref[ref["arfcn"] == i]
        assert sum(bool(_is_imm_ass(r)) for r in mine) == len(ia)
        per_tn = [int(np.sum((mine["type"] >= 0x10) & (mine["tn"] == tn))) for _, tn, _ in ia]
        assert min(per_tn) >= 10, per_tn
    n = cap["x"].shape[1]
    for sizes in ([], [936] * (n // 936 + 1)):
        rec, status, chains, pushes = cases.stream(gpu_api, cap["x"], cap["t"], cap["kc"], sizes, arfcn)
        _check_same(gpu_api, "reassigned", cap, arfcn, rec, status, chains)
        if sizes:
            assert max(sum(bool(_is_imm_ass(r)) for r in p[p["arfcn"] == 1]) for p in pushes) == 1


@pytest.mark.timeout(300)
def test_stream_without_traffic(gpu_api, pkg):
    """A handle that follows TCH3 calls, fed an all-zero traffic carrier, gives the plain stream's records; the plain
    handle's are what they were: gmr1_hip_rx_run's."""
    x = plain._carriers(pkg)
    arfcn = np.arange(x.shape[0], dtype=np.uint16) + 200
    sizes = [20000] * (x.shape[1] // 20000 + 1)
    rec, status, chains, _ = plain._stream(gpu_api, x, sizes, arfcn)
    ref = plain._check_same(gpu_api, x, arfcn, rec, status, chains)
    assert len(ref) > 200
    rec_t, status_t, chains_t, _ = cases.stream(gpu_api, x, np.zeros_like(x), None, sizes, arfcn)
    assert np.array_equal(status_t, status) and np.array_equal(chains_t, chains)
    assert plain._sorted(rec_t, arfcn).tobytes() == ref.tobytes()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_batched_assign_is_the_host_assign_in_order(gpu_api, pkg):
    """64 random states; `call` names some twice, some three times and some never, over more than one work-group"""
    import torch
    api = gpu_api
    rng = np.random.default_rng(41)
    state = np.frombuffer(rng.integers(0, 256, 64 * api.TCH3_STATE.itemsize, dtype=np.uint8).tobytes(), api.TCH3_STATE).copy()
    state["energy_dkab"] = rng.random(64, dtype=np.float32)        # (no NaN patterns: bytes are compared)
    state["energy_burst"] = rng.random(64, dtype=np.float32)
    call = np.concatenate([rng.permutation(64)[:40], rng.integers(0, 20, 30), [-1, 63, 63]]).astype(np.int32)
    named = set(int(c) for c in call if c >= 0)
    assert len(named) < 64 and max(np.bincount(call[call >= 0])) >= 3 and call.size > 64
    p = rng.integers(0, 40, call.size).astype(np.int32)
    en = (rng.random(call.size, dtype=np.float32) * 3).astype(np.float32)
    want = state.copy()
    for c, pp, e in zip(call, p, en):
        if c >= 0:
            api.tch3_state_assign(want, int(pp), float(e), index=int(c))
    d_state, d_call, d_p, d_en = _dev(torch, state), _dev(torch, call), _dev(torch, p), _dev(torch, en)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.tch3_state_assign_batch_dev(st.cuda_stream, call.size, d_call.data_ptr(), d_p.data_ptr(), d_en.data_ptr(), d_state.data_ptr())
    st.synchronize()
    got = np.frombuffer(d_state.cpu().numpy().tobytes(), api.TCH3_STATE)
    assert got.tobytes() == want.tobytes()
    for k in range(64):
        if k not in named:
            assert got[k].tobytes() == state[k].tobytes()
    # nothing to do, and what is refused: the states stay
    api.tch3_state_assign_batch_dev(st.cuda_stream, 0, d_call.data_ptr(), d_p.data_ptr(), d_en.data_ptr(), d_state.data_ptr())
    f = api._fn("gmr1_hip_tch3_state_assign_batch_dev")
    assert f(None, -1, d_call.data_ptr(), d_p.data_ptr(), d_en.data_ptr(), d_state.data_ptr()) == -22
    assert f(None, 1, None, d_p.data_ptr(), d_en.data_ptr(), d_state.data_ptr()) == -22
    assert f(None, 1, d_call.data_ptr(), d_p.data_ptr(), d_en.data_ptr(), None) == -22
    st.synchronize()
    assert d_state.cpu().numpy().tobytes() == want.tobytes()


def test_follower_with_a_device_side_assign_between_invocations(gpu_api, pkg):
    """One call, its frames in two gmr1_hip_tch3_follow_batch_dev invocations with an assignment between them that runs on
    the device: the state never leaves it, and the records are those of the route through the host's assign."""
    import torch
    api = gpu_api
    car = tc.carrier(pkg, tc.CIPHERED)
    iq, first, offset, fs, fn = tc.pack([car])
    n, cut = offset.size, offset.size // 2
    p2, e2 = (car["p"] + 3) % 40, 0.9
    st0 = tc.initial_state(pkg, car)
    a, mid = api.tch3_follow(iq, [0, cut], offset[:cut], fs[:cut], fn[:cut], st0, sps=car["sps"])
    api.tch3_state_assign(mid, p2, e2)
    b, end = api.tch3_follow(iq, [0, n - cut], offset[cut:], fs[cut:], fn[cut:], mid, sps=car["sps"])
    want = np.concatenate([a, b])
    assert (want["type"] != 0).sum() > 10

    d = dict(iq=_dev(torch, iq), off=_dev(torch, offset), fs=_dev(torch, fs), fn=_dev(torch, fn), state=_dev(torch, st0),
             first=[_dev(torch, np.array([0, cut], np.int32)), _dev(torch, np.array([0, n - cut], np.int32))],
             call=_dev(torch, np.array([0], np.int32)), p=_dev(torch, np.array([p2], np.int32)),
             en=_dev(torch, np.array([e2], np.float32)), out=torch.zeros(n * 40, dtype=torch.uint8, device="cuda"))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = st.cuda_stream
    api.tch3_follow_dev(s, 1, cut, d["iq"].data_ptr(), d["first"][0].data_ptr(), d["off"].data_ptr(), d["fs"].data_ptr(),
                        d["fn"].data_ptr(), d["state"].data_ptr(), d["out"].data_ptr(), sps=car["sps"])
    api.tch3_state_assign_batch_dev(s, 1, d["call"].data_ptr(), d["p"].data_ptr(), d["en"].data_ptr(), d["state"].data_ptr())
    api.tch3_follow_dev(s, 1, n - cut, d["iq"].data_ptr(), d["first"][1].data_ptr(), d["off"].data_ptr() + 8 * cut,
                        d["fs"].data_ptr() + 4 * cut, d["fn"].data_ptr() + 4 * cut, d["state"].data_ptr(),
                        d["out"].data_ptr() + 40 * cut, sps=car["sps"])
    st.synchronize()
    assert d["out"].cpu().numpy().tobytes() == want.tobytes()
    assert d["state"].cpu().numpy().tobytes() == end.tobytes()


@pytest.mark.timeout(300)
def test_stream_tch_retention_is_bounded(gpu_api, pkg):
    """At 10 ms pushes a live carrier never holds more than a push, four frames and the drop granule -- of both its BCCH
    and its traffic samples: the two buffers share one `retained` (_status), stride and growth.  That the second pair, the
    call states and the staging blocks do not grow is read off the device: once every call is under way (2.5 s in: pushes
    of this size, with call frames, have been made for a second) the device's free memory is the same after every push."""
    import torch
    cap = cases.pairs(pkg)
    A, n = cap["x"].shape
    arfcn = np.arange(A, dtype=np.uint16)
    seen, free = [], []

    def after_push(s, at):
        status, chains, retained = s.status()
        if at >= plain.H_ACQ:
            live = (status == 0) & (chains > 0)
            assert live.sum() >= 4
            assert (retained[live] <= 936 + 4 * FRAME + 64).all(), retained.max()
            assert (retained[~live] == 0).all()
            seen.append(int(retained.max()))
        else:
            assert (retained == at).all()
        if at >= int(2.5 * 23400 * SPS):
            free.append(torch.cuda.mem_get_info()[0])

    with gpu_api.RxStream(A, sps=SPS, arfcn=arfcn, tch=True, kc=cap["kc"]) as s:
        for at in range(0, n, 936):
            k = min(936, n - at)
            s.push(cap["x"][:, at:at + k], tch=cap["t"][:, at:at + k], last=at + k >= n)
            if at + k < n:
                after_push(s, at + k)
        assert (s.status()[2] == 0).all()
    assert len(seen) > 100
    assert len(free) > 100 and len(set(free)) == 1, sorted(set(free))


def test_rx_run_tch_dev_is_rx_run_tch(gpu_api, pkg):
    """the device-pointer form of the one-shot call (what tools/time_rx_stream.py --tch measures against)"""
    import torch
    cap = cases.pairs(pkg)
    A, n = cap["x"].shape
    arfcn = np.arange(A, dtype=np.uint16) + 200
    ref, rst, rch = cases.one_shot(gpu_api, "pairs", cap, arfcn)
    d_x, d_t = _dev(torch, cap["x"]), _dev(torch, cap["t"])
    torch.cuda.synchronize()
    offset = np.arange(A, dtype=np.uint64) * np.uint64(n)
    rec, status, chains, found = gpu_api.rx_run_tch_dev(torch.cuda.current_stream().cuda_stream, d_x.data_ptr(), d_t.data_ptr(), offset,
                                                        np.full(A, n, np.uint64), sps=SPS, arfcn=arfcn, kc=cap["kc"], max_records=1 << 20)
    assert found == len(rec) and rec.tobytes() == ref.tobytes()
    assert np.array_equal(status, rst) and np.array_equal(chains, rch)


@pytest.mark.timeout(300)
def test_stream_tch_refusals_leave_the_handle_unchanged(gpu_api, pkg):
    api = gpu_api
    cap = cases.pairs(pkg)
    x, t, kc = (np.ascontiguousarray(cap[k][:2]) for k in ("x", "t", "kc"))
    arfcn = np.array([0, 1], np.uint16)
    two = dict(x=x, t=t, kc=kc)
    ref, rst, rch = cases.one_shot(api, "pairs[:2]", two, arfcn)
    assert (ref["type"] >= 0x10).sum() > 20
    push, push_tch = api._fn("gmr1_hip_rx_stream_push"), api._fn("gmr1_hip_rx_stream_push_tch")
    n, step = x.shape[1], 60000
    got_n = C.c_int(7)
    with api.RxStream(2, sps=SPS, arfcn=arfcn, tch=True, kc=kc) as s, api.RxStream(2, sps=SPS, arfcn=arfcn) as s0:
        got, got0 = [], []
        for at in range(0, n, step):
            k = min(step, n - at)
            xa, ta = np.ascontiguousarray(x[:, at:at + k]), np.ascontiguousarray(t[:, at:at + k])
            m = s.max_records(k)
            assert m > s0.max_records(k) or m == 0
            out = np.empty(max(m, 1), api.RX_RECORD)
            # the plain entry on a tch handle, the tch entry on a plain handle, no traffic samples, a buffer below the bound
            assert push(s._h, xa.ctypes.data, k, k, 0, out.ctypes.data, out.size, C.byref(got_n)) == -22 and got_n.value == 0
            assert push_tch(s0._h, xa.ctypes.data, ta.ctypes.data, k, k, 0, out.ctypes.data, out.size, C.byref(got_n)) == -22
            assert push_tch(s._h, xa.ctypes.data, None, k, k, 0, out.ctypes.data, out.size, C.byref(got_n)) == -22
            if m > 1:
                assert push_tch(s._h, xa.ctypes.data, ta.ctypes.data, k, k, 0, out.ctypes.data, m - 1, C.byref(got_n)) == -22
            with pytest.raises(ValueError):
                s.push(xa)
            with pytest.raises(ValueError):
                s0.push(xa, tch=ta)
            got.append(s.push(xa, tch=ta, last=at + k >= n).copy())
            got0.append(s0.push(xa, last=at + k >= n).copy())
        status, chains, _ = s.status()
    mine = plain._sorted(np.concatenate(got), arfcn)
    assert np.array_equal(status, rst) and np.array_equal(chains, rch)
    assert mine.tobytes() == ref.tobytes()
    assert plain._sorted(np.concatenate(got0), arfcn).tobytes() == ref[ref["type"] < 0x10].tobytes()
