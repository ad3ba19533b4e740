"""GPU tests of the streaming receive loop with the TCH3 and TCH9 follow-ups (gmr1_hip_rx_stream_create_full /
_push_full*): any sequence of pushes gives, once sorted by (carrier, chain), byte for byte the records and the big records
of one gmr1_hip_rx_run_full call on the same samples with the same keys, and its status / n_chains; and of k_tch9f_big
(gmr1_hip_tch9_frames_to_records_dev), which closes the follower's frames up into big records on the device."""
import ctypes as C

import numpy as np
import pytest

import rx_stream_full_cases as cases
import test_gpu_rx_stream as plain

pytestmark = pytest.mark.gpu

SPS = cases.SPS
FRAME = cases.FRAME


def _is_ass_cmd(r):
    return r["type"] == 0x12 and r["l2"][3] == 0x06 and r["l2"][4] == 0x2e


def _check_same(api, name, cap, arfcn, rec, big, status, chains, sps=SPS):
    ref, ref_big, rst, rch = cases.one_shot(api, name, cap, arfcn, sps)
    assert np.array_equal(status, rst), (status, rst)
    assert np.array_equal(chains, rch), (chains, rch)
    mine, mine_big = plain._sorted(rec, arfcn), plain._sorted(big, arfcn)
    assert len(mine) == len(ref), (len(mine), len(ref))
    assert mine.tobytes() == ref.tobytes(), "streamed records differ from the one-shot call's"
    assert len(mine_big) == len(ref_big), (len(mine_big), len(ref_big))
    assert mine_big.tobytes() == ref_big.tobytes(), "streamed big records differ from the one-shot call's"
    return ref, ref_big


def _ordered(pushes):
    """within a push both arrays come by carrier, chain (and, being identical to the one-shot's once sorted, by frame)"""
    for rec, big in pushes:
        for p in (rec, big):
            key = p["arfcn"].astype(np.int64) * 256 + p["chain"]
            assert (np.diff(key) >= 0).all()


def _schedule(name, n):
    if name == "one":
        return []
    if name == "10ms":
        return [936] * (n // 936 + 1)
    if name == "frame":
        return [FRAME] * (n // FRAME + 1)
    rng = np.random.default_rng(19)
    s = []
    while sum(s) < n:
        s.append(0 if len(s) % 10 == 4 else int(rng.integers(0, 3 * FRAME + 1)))
    return s


@pytest.mark.timeout(600)
@pytest.mark.parametrize("sched", ["one", "10ms", "frame", "random"])
def test_stream_full_matches_one_shot(gpu_api, pkg, orc, decoder, sched):
    """The three carriers of test_rx_loop_tch9_follow_up_matches_oracle: TCH9 only, FACCH9 / TCH9 without a key, and
    ciphered on timeslot 17."""
    cap = cases.triples(pkg, orc)
    A, n = cap["x"].shape
    arfcn = np.arange(A, dtype=np.uint16) + 200
    # the input, judged on the one-shot result
    ref, ref_big, _, _ = cases.one_shot(gpu_api, "triples", cap, arfcn)
    assert len(ref_big) > 100
    for a in arfcn:
        assert int(np.sum(ref_big["arfcn"] == a)) >= 20
        assert sum(bool(_is_ass_cmd(r)) for r in ref[ref["arfcn"] == a]) > 1
    rec, big, status, chains, pushes = cases.stream(gpu_api, cap, _schedule(sched, n), arfcn)
    _check_same(gpu_api, "triples", cap, arfcn, rec, big, status, chains)
    _ordered(pushes)
    if sched == "10ms":
        assert sum(bool(len(b)) for _, b in pushes) >= 2, "big records should come out as the call goes on"
        for a in arfcn:
            first_big = next(i for i, (_, b) in enumerate(pushes) if (b["arfcn"] == a).any())
            first_cmd = next(i for i, (r, _) in enumerate(pushes) if any(_is_ass_cmd(q) for q in r[r["arfcn"] == a]))
            assert first_big == first_cmd, (int(a), first_big, first_cmd)


@pytest.mark.timeout(600)
def test_stream_full_two_timeslots_on_one_chain(gpu_api, pkg, orc, decoder):
    """Commands to timeslot 5 and then to timeslot 14 on one chain: in one push (every command a call of the follower's one
    invocation), at 10 ms (a command per push at the most, the call before it carried in) and at 1 s."""
    cap = cases.two_slots(pkg, orc)
    n = cap["x"].shape[1]
    arfcn = np.array([7], np.uint16)
    ref, ref_big, _, _ = cases.one_shot(gpu_api, "two_slots", cap, arfcn)
    per_tn = [int(np.sum(ref_big["tn"] == tn9)) for _, tn9 in cases.TWO_SLOTS]
    assert min(per_tn) >= 10 and sum(per_tn) == len(ref_big), (per_tn, len(ref_big))
    for sizes in ([], [936] * (n // 936 + 1), [23400 * SPS] * (n // (23400 * SPS) + 1)):
        rec, big, status, chains, pushes = cases.stream(gpu_api, cap, sizes, arfcn)
        _check_same(gpu_api, "two_slots", cap, arfcn, rec, big, status, chains)
        _ordered(pushes)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("sps", [2, 11])
def test_stream_full_at_other_sps(gpu_api, pkg, orc, sps):
    cap = cases.at_sps(pkg, orc, sps)
    n = cap["x"].shape[1]
    arfcn = np.array([3], np.uint16)
    _, ref_big, _, _ = cases.one_shot(gpu_api, "sps%d" % sps, cap, arfcn, sps)
    assert len(ref_big) > 20
    frame = 24 * 39 * sps
    for sizes in ([], [frame] * (n // frame + 1)):
        rec, big, status, chains, _ = cases.stream(gpu_api, cap, sizes, arfcn, sps=sps)
        _check_same(gpu_api, "sps%d" % sps, cap, arfcn, rec, big, status, chains, sps)


def test_create_full_refuses_sps_12(gpu_api):
    h = C.c_void_p(5)
    assert gpu_api._fn("gmr1_hip_rx_stream_create_full")(2, 12, None, None, C.byref(h)) == -22 and h.value is None
    with gpu_api.RxStream(2, sps=11, full=True) as s:
        assert s.max_big(100) == 2 * 16 * 2 and s.max_records(100) > 0


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.timeout(300)
def test_push_full_dev_gives_the_host_forms_bytes(gpu_api, pkg, orc):
    """the samples in device memory, carrier rows a whole capture apart, read on a stream of the caller's"""
    import torch
    cap = cases.triples(pkg, orc)
    A, n = cap["x"].shape
    arfcn = np.arange(A, dtype=np.uint16) + 200
    sizes = [9360] * (n // 9360 + 1)
    _, _, status, chains, host = cases.stream(gpu_api, cap, sizes, arfcn)
    d = [_dev(torch, cap[k]) for k in ("x", "t", "c")]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    at = [0]

    def push(s, xa, ta, ca, last):
        k = xa.shape[1]
        r = s.push_dev(st.cuda_stream, d[0].data_ptr() + 8 * at[0], n, k, last=last, tch_ptr=d[1].data_ptr() + 8 * at[0],
                       csd_ptr=d[2].data_ptr() + 8 * at[0])
        at[0] += k
        return r

    _, _, status_d, chains_d, dev = cases.stream(gpu_api, cap, sizes, arfcn, push=push)
    assert np.array_equal(status, status_d) and np.array_equal(chains, chains_d)
    assert len(dev) == len(host) and sum(len(b) for _, b in host) > 100
    for (r, b), (rd, bd) in zip(host, dev):
        assert r.tobytes() == rd.tobytes() and b.tobytes() == bd.tobytes()


@pytest.mark.timeout(300)
def test_stream_full_refusals_leave_the_handle_unchanged(gpu_api, pkg, orc):
    """every refusal of the contract between real pushes: the counts are 0, and the handle goes on and ends identical"""
    api = gpu_api
    cap = cases.triples(pkg, orc)
    two = {k: np.ascontiguousarray(v[:2]) for k, v in cap.items()}
    arfcn = np.array([0, 1], np.uint16)
    ref, ref_big, _, _ = cases.one_shot(api, "triples[:2]", two, arfcn)
    assert len(ref_big) > 40
    push, push_tch, push_full = (api._fn("gmr1_hip_rx_stream_push" + k) for k in ("", "_tch", "_full"))
    n, step = two["x"].shape[1], 60000
    n_rec, n_big = C.c_int(7), C.c_int(7)

    def refused(rv):
        ok = rv == -22 and n_rec.value == 0 and n_big.value in (0, 7)
        n_rec.value = 7
        return ok

    with api.RxStream(2, sps=SPS, arfcn=arfcn, full=True, kc=two["kc"]) as s, api.RxStream(2, sps=SPS, arfcn=arfcn) as s0, \
            api.RxStream(2, sps=SPS, arfcn=arfcn, tch=True, kc=two["kc"]) as s1:
        got = []
        for at in range(0, n, step):
            k = min(step, n - at)
            xa, ta, ca = (np.ascontiguousarray(two[key][:, at:at + k]) for key in ("x", "t", "c"))
            px, pt, pc = xa.ctypes.data, ta.ctypes.data, ca.ctypes.data
            m, mb = s.max_records(k), s.max_big(k)
            assert s0.max_big(k) == 0 and s1.max_big(k) == 0
            if at == 0:            # (the other two handles stay where they are: only here are all three in one state)
                assert m == s1.max_records(k) > s0.max_records(k)
            assert mb == int(s.status()[1].sum() if at >= plain.H_ACQ else 32) * ((int(s.status()[2].max()) + k) // FRAME + 2)
            out, big = np.empty(max(m, 1), api.RX_RECORD), np.empty(max(mb, 1), api.RX_BIG_RECORD)
            po, pb = out.ctypes.data, big.ctypes.data
            tail = (po, out.size, C.byref(n_rec), pb, big.size, C.byref(n_big))
            # the other entries on a full handle, the full entry on the other handles
            assert refused(push(s._h, px, k, k, 0, po, out.size, C.byref(n_rec)))
            assert refused(push_tch(s._h, px, pt, k, k, 0, po, out.size, C.byref(n_rec)))
            n_big.value = 7
            assert refused(push_full(s0._h, px, pt, pc, k, k, 0, *tail)) and n_big.value == 0
            n_big.value = 7
            assert refused(push_full(s1._h, px, pt, pc, k, k, 0, *tail)) and n_big.value == 0
            # no traffic samples, no CSD samples, buffers below their bounds, no big buffer
            for args in ((px, None, pc), (px, pt, None)):
                n_big.value = 7
                assert refused(push_full(s._h, *args, k, k, 0, *tail)) and n_big.value == 0
            if mb > 1:
                n_big.value = 7
                assert refused(push_full(s._h, px, pt, pc, k, k, 0, po, out.size, C.byref(n_rec), pb, mb - 1, C.byref(n_big)))
                assert n_big.value == 0
            if mb > 0:
                assert refused(push_full(s._h, px, pt, pc, k, k, 0, po, out.size, C.byref(n_rec), None, mb, C.byref(n_big)))
            if m > 1:
                assert refused(push_full(s._h, px, pt, pc, k, k, 0, po, m - 1, C.byref(n_rec), pb, big.size, C.byref(n_big)))
            for kw in (dict(), dict(tch=ta), dict(csd=ca)):
                with pytest.raises(ValueError):
                    s.push(xa, **kw)
            with pytest.raises(ValueError):
                s1.push(xa, tch=ta, csd=ca)
            r, b = s.push(xa, tch=ta, csd=ca, last=at + k >= n)
            got.append((r.copy(), b.copy()))
        status, chains, _ = s.status()
    _check_same(api, "triples[:2]", two, arfcn, np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]), status, chains)


@pytest.mark.timeout(300)
def test_stream_full_retention_is_bounded(gpu_api, pkg, orc):
    """At 10 ms pushes a live carrier never holds more than a push, four frames and the drop granule -- of its BCCH, traffic
    and CSD samples alike: the three buffers share one `retained` (_status), stride and growth.  That the third pair, the
    call states and the follower's scratch do not grow is read off the device: once every data call is under way (4 s in:
    pushes of this size, with NT9 frames, have been made for a second) the device's free memory is the same after every
    push."""
    import torch
    cap = cases.triples(pkg, orc)
    A, n = cap["x"].shape
    arfcn = np.arange(A, dtype=np.uint16)
    seen, free, bigs = [], [], []

    def after_push(s, at):
        status, chains, retained = s.status()
        if at >= plain.H_ACQ:
            live = (status == 0) & (chains > 0)
            assert live.all()
            assert (retained[live] <= 936 + 4 * FRAME + 64).all(), retained.max()
            seen.append(int(retained.max()))
        else:
            assert (retained == at).all()
        if at >= int(4.0 * 23400 * SPS):
            free.append(torch.cuda.mem_get_info()[0])

    _, big, _, _, pushes = cases.stream(gpu_api, cap, [936] * (n // 936 + 1), arfcn, after_push=after_push)
    first_big = next(i for i, (_, b) in enumerate(pushes) if len(b))
    assert (first_big + 1) * 936 < int(3.0 * 23400 * SPS) and len(big) > 100
    assert len(seen) > 100
    assert len(free) > 100 and len(set(free)) == 1, sorted(set(free))


def _want_big(api, first, frames, label):
    keep = [(c, k) for c in range(len(label)) for k in range(first[c], first[c + 1]) if frames["type"][k]]
    out = np.zeros(len(keep), api.RX_BIG_RECORD)
    for i, (c, k) in enumerate(keep):
        out["arfcn"][i], out["chain"][i], out["tn"][i] = label[c] & 0xffff, (label[c] >> 16) & 0xff, label[c] >> 24
        for name in ("fn", "type", "len", "conv"):
            out[name][i] = frames[name][k]
        out["l2"][i, :frames["len"][k]] = frames["l2"][k, :frames["len"][k]]
    return out


def test_frames_to_records_is_the_numpy_restatement(gpu_api):
    """k_tch9f_big alone: calls of 0, 1, 63, 64, 65, 130 and 0 frames and one whose frames all have type 0, over more
    than one work-group; every field of a frame random, l2 beyond len included"""
    import torch
    api = gpu_api
    rng = np.random.default_rng(90)
    counts = [0, 1, 63, 64, 70, 65, 130, 0, 5]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n = int(first[-1])
    frames = np.frombuffer(rng.integers(0, 256, n * api.TCH9_FRAME.itemsize, dtype=np.uint8).tobytes(), api.TCH9_FRAME).copy()
    frames["type"] = rng.choice(np.array([0, 0x18, 0x1a], np.uint8), n)
    frames["len"] = rng.integers(0, 65, n)
    frames["type"][first[4]:first[5]] = 0            # the call of 70 frames reports nothing
    label = rng.integers(0, 1 << 32, len(counts), dtype=np.uint64).astype(np.uint32)
    want = _want_big(api, first, frames, label)
    assert 150 < len(want) < n and (frames["len"] == 64).any() and (frames["len"] < 4).any()
    d_first, d_frames, d_label = _dev(torch, first), _dev(torch, frames), _dev(torch, label)
    st = torch.cuda.Stream()
    for max_out in (n, len(want), len(want) - 3, 0):
        d_out = torch.full(((max_out + 2) * 80,), 0xEE, dtype=torch.uint8, device="cuda")
        d_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        api.tch9_frames_to_records_dev(st.cuda_stream, len(counts), d_first.data_ptr(), n, d_frames.data_ptr(), d_label.data_ptr(),
                                       d_out.data_ptr() if max_out else None, max_out, d_n.data_ptr())
        st.synchronize()
        assert int(d_n.item()) == len(want)
        got = d_out.cpu().numpy()
        fit = min(max_out, len(want))
        assert got[:fit * 80].tobytes() == want[:fit].tobytes()
        assert (got[fit * 80:] == 0xEE).all(), "a record past max_out, or past the count, was written"
    # no call at all: the count is written, nothing else
    d_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    d_out = torch.full((160,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    api.tch9_frames_to_records_dev(st.cuda_stream, 0, d_first.data_ptr(), 0, d_frames.data_ptr(), d_label.data_ptr(), d_out.data_ptr(), 2,
                                   d_n.data_ptr())
    st.synchronize()
    assert int(d_n.item()) == 0 and (d_out.cpu().numpy() == 0xEE).all()
