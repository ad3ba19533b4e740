"""The batched TCH9 call follower (gmr1_hip_tch9_follow*) on the GPU against the walk of tests/tch9_cases.py over the CPU
oracle's primitives (rx_tch9, reference src/gmr1_rx.c:262-353).  Everything behind the demodulator is integer arithmetic:
every field of every record and every byte of every state must be equal."""
import threading

import numpy as np
import pytest

import tch9_cases as t9

pytestmark = pytest.mark.gpu

FIELDS = ("cls", "type", "len", "crc", "fn", "conv", "l2", "pad")


def same_records(got, want, what=""):
    assert got.shape == want.shape, what
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, [k for k in range(len(got)) if not np.array_equal(got[f][k], want[f][k])][:8])
    assert got.tobytes() == want.tobytes(), what


def same_states(got, want, what=""):
    for f in ("active", "n_held", "kc", "held"):
        assert np.array_equal(got[f], want[f]), (what, f)
    assert got.tobytes() == want.tobytes(), what


def run_batch(api, b, mode):
    return api.tch9_follow_bits(b["first"], b["ebits"], b["sync_id"], b["fn"], b["state"], rv=b["rv"], mode=mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bits_form_against_the_oracle(gpu_api, pkg, orc, decoder, mode):
    """Five calls of 9, 0, 5, 1 and 4 frames in one invocation, FACCH9, TCH9 and refused windows mixed, the last call not
    active: every record and every state."""
    b = t9.batch(pkg, orc, mode)
    want, want_state = t9.batch_expected(pkg, orc, mode)
    out, state = run_batch(gpu_api, b, mode)
    same_records(out, want, (decoder, mode))
    same_states(state, want_state, (decoder, mode))
    # the call without frames and the inactive one keep their states byte for byte
    assert state[1].tobytes() == b["state"][1].tobytes() and state[4].tobytes() == b["state"][4].tobytes()
    first = b["first"]
    assert (out["cls"][first[4]:] == t9.OFF).all() and not out["type"][first[4]:].any()
    seen = set()
    for c, call in enumerate(b["calls"][:4]):
        rec = out[first[c]:first[c + 1]]
        seen |= set(int(x) for x in rec["cls"])
        t_idx = [k for k, kind in enumerate(call["kinds"]) if kind == "T"]
        for j, k in enumerate(t_idx):
            assert rec["type"][k] == 0x18 and rec["len"][k] == t9.TCH9_BYTES[mode]
            if j >= 2:                                   # a TCH9 block is what was sent two TCH9 bursts earlier
                assert bytes(rec["l2"][k][:t9.TCH9_BYTES[mode]]) == bytes(call["sent"][t_idx[j - 2]]), (c, k)
        for k, kind in enumerate(call["kinds"]):
            if kind == "F":                              # the encoded FACCH9 messages pass their CRC
                assert rec["type"][k] == 0x1a and rec["crc"][k] == 0 and bytes(rec["l2"][k][:38]) == bytes(call["sent"][k]), (c, k)
    assert seen == {t9.FACCH9, t9.TCH9, t9.ERR}
    # rv left out means every window was accepted: the E frames count as TCH9 bursts (their sync_id is 1)
    out0, _ = gpu_api.tch9_follow_bits(b["first"], b["ebits"], b["sync_id"], b["fn"], b["state"], rv=None, mode=mode)
    assert not (out0["cls"] == t9.ERR).any() and (out0["cls"][:first[4]] == t9.TCH9).sum() == (b["sync_id"][:first[4]] != 0).sum()


def _nine(pkg, orc, mode=2):
    call = t9.batch(pkg, orc, mode)["calls"][t9.NINE]
    n = len(call["fn"])
    want, held = t9.expected_run(pkg, orc, mode, [call["kc"]] * n, call["ebits"], call["sync_id"], call["rv"], call["fn"])
    return call, n, want, held


def _piece(api, call, lo, hi, state, mode=2):
    return api.tch9_follow_bits([0, hi - lo], call["ebits"][lo:hi], call["sync_id"][lo:hi], call["fn"][lo:hi], state,
                                rv=call["rv"][lo:hi], mode=mode)


def test_a_call_continued(gpu_api, pkg, orc, decoder):
    """The 9-frame call cut at each of its 10 positions, and once into three pieces with an empty one, the state passed
    through host memory: records and final state are those of the one invocation and of the oracle, byte for byte."""
    api = gpu_api
    call, n, want, held = _nine(pkg, orc)
    whole, whole_state = _piece(api, call, 0, n, t9.fresh_state(pkg, call["kc"]))
    same_records(whole, want, decoder)
    same_states(whole_state, t9.state_of(pkg, call["kc"], 1, held[n]), decoder)
    n_held_at_cut, kind_at_cut = set(), set()
    for cuts in [[0, p, n] for p in range(n + 1)] + [[0, 3, 3, 6, n]]:
        state = t9.fresh_state(pkg, call["kc"])
        pieces = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            out, state = _piece(api, call, lo, hi, state)
            same_states(state, t9.state_of(pkg, call["kc"], 1, held[hi]), (cuts, hi))
            pieces.append(out)
        assert np.concatenate(pieces).tobytes() == whole.tobytes(), cuts
        assert state.tobytes() == whole_state.tobytes(), cuts
        if len(cuts) == 3:
            n_held_at_cut.add(held[cuts[1]][0])
            kind_at_cut |= {call["kinds"][cuts[1] - 1:cuts[1]], call["kinds"][cuts[1]:cuts[1] + 1]}
    # by construction: a cut that leaves one burst held, and FACCH9 / refused frames right at a cut
    assert n_held_at_cut == {0, 1, 2} and {"F", "E", "T"} <= kind_at_cut


def test_state_semantics(gpu_api, pkg, orc):
    """Re-assigned in the middle, the next TCH9 block decodes against zeros as the oracle's fresh interleaver does; a key
    changed between two invocations deciphers only what is taken in after it; with a wrong key a FACCH9 fails its CRC."""
    api = gpu_api
    mode = 2
    call, n, _, _ = _nine(pkg, orc)
    run = lambda keys, lo, hi: t9.expected_run(pkg, orc, mode, keys, call["ebits"][lo:hi], call["sync_id"][lo:hi], call["rv"][lo:hi],
                                               call["fn"][lo:hi])
    # re-assign at frame 5: two runs of the oracle
    cut = 5
    out1, st = _piece(api, call, 0, cut, t9.fresh_state(pkg, call["kc"]))
    assert st["n_held"][0] == 2
    st = api.tch9_state_assign(st)
    out2, st = _piece(api, call, cut, n, st)
    w1, _ = run([call["kc"]] * cut, 0, cut)
    w2, h2 = run([call["kc"]] * (n - cut), cut, n)
    same_records(np.concatenate([out1, out2]), np.concatenate([w1, w2]), "re-assign")
    same_states(st, t9.state_of(pkg, call["kc"], 1, h2[-1]), "re-assign")

    # another key from frame 3 on (frame 2 is a TCH9 burst taken in under the first key: it stays deciphered with that one)
    other = call["kc"] ^ np.uint8(0x5a)
    cut = 3
    keys = [call["kc"]] * cut + [other] * (n - cut)
    want, held = run(keys, 0, n)
    out1, st = _piece(api, call, 0, cut, t9.fresh_state(pkg, call["kc"]))
    assert st["n_held"][0] == 2
    st["kc"][0] = other
    out2, st = _piece(api, call, cut, n, st)
    same_records(np.concatenate([out1, out2]), want, "key change")
    same_states(st, t9.state_of(pkg, other, 1, held[n]), "key change")
    # (and it matters: the whole run under either key alone gives other records)
    assert np.concatenate([out1, out2]).tobytes() != run([call["kc"]] * n, 0, n)[0].tobytes()

    # a wrong key: the FACCH9 messages fail their CRC and report nothing but that and the decoder's value
    wrong = call["kc"] ^ np.uint8(0xff)
    out, _ = _piece(api, call, 0, n, t9.fresh_state(pkg, wrong))
    want_w, _ = run([wrong] * n, 0, n)
    same_records(out, want_w, "wrong key")
    fa = out[[k for k, kind in enumerate(call["kinds"]) if kind == "F"]]
    assert len(fa) == 2 and (fa["cls"] == t9.FACCH9).all() and (fa["crc"] == 1).all() and not fa["type"].any() and not fa["l2"].any()


def _pack(cars):
    base, pos = [], 0
    for c in cars:
        base.append(pos)
        pos += (c["x"].size + 15) & ~15
    iq = np.zeros(pos, np.complex64)
    for b, c in zip(base, cars):
        iq[b:b + c["x"].size] = c["x"]
    first = np.concatenate([[0], np.cumsum([c["offset"].size for c in cars])]).astype(np.int32)
    offset = np.concatenate([c["offset"] + np.uint64(b) for b, c in zip(base, cars)]).astype(np.uint64)
    return iq, first, offset, np.concatenate([c["freq_shift"] for c in cars]), np.concatenate([c["fn"] for c in cars])


@pytest.mark.parametrize("sps", [4, 2, 11])
def test_from_samples(gpu_api, pkg, orc, sps):
    """Two carriers as two calls of one invocation, TCH9 bursts, idle frames and bursts sent with sync sequence 0, a carrier
    offset taken out by freq_shift: (a) what the bits form gives on gmr1_hip_demod_batch's output for the same windows,
    exactly; (b) the oracle's walk from its own demodulation of every frame -- the inputs are chosen on the oracle alone so
    that no frame's decision is within rounding of flipping, which is asserted first."""
    api = gpu_api
    specs = t9.CARRIERS[sps]
    cars = [t9.carrier(pkg, orc, *s) for s in specs]
    dems = [t9.carrier_demod(pkg, orc, *s) for s in specs]
    for s, d in zip(specs, dems):
        assert t9.carrier_margin_ok(sps, d) == [], s
        assert len(d) >= 20
    for c in cars:
        assert {"tch9", "idle", "facch9"} <= set(c["sent"])
    iq, first, offset, fs, fn = _pack(cars)
    state = np.concatenate([t9.fresh_state(pkg, c["kc"]) for c in cars])
    out, st = api.tch9_follow(iq, first, offset, fs, fn, state, sps=sps)

    # (a) plumbing: the demodulator's own output through the bits form
    d = api.demod_batch("nt9", iq, offset, t9.in_len(sps), sps=sps, freq_shift=fs)
    out_b, st_b = api.tch9_follow_bits(first, d["ebits"], d["sync_id"], fn, state, rv=d["rv"])
    assert out.tobytes() == out_b.tobytes() and st.tobytes() == st_b.tobytes()

    # (b) the oracle: its demodulation, its keystreams, its decoders
    with orc.conv_mode(1 if api.get_conv_decoder() == api.CONV_ACC else 0):
        for c, (car, dem) in enumerate(zip(cars, dems)):
            n = len(dem)
            eb = np.array([b["ebits"] for b, _, _ in dem], np.int8)
            sid = np.array([b["sync_id"] for b, _, _ in dem], np.int32)
            want, held = t9.expected_run(pkg, orc, 2, [car["kc"]] * n, eb, sid, np.zeros(n, np.int32), car["fn"])
            same_records(out[first[c]:first[c + 1]], want, (sps, c))
            same_states(st[c:c + 1], t9.state_of(pkg, car["kc"], 1, held[n]), (sps, c))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_dev_forms_equal_the_host_forms(gpu_api, pkg, orc):
    """Everything in device memory, on a stream of the caller's: the host forms' bytes.  And rx_tch9_init on device-resident
    states: a call named twice, a negative index."""
    import torch
    api = gpu_api
    mode = 2
    b = t9.batch(pkg, orc, mode)
    want_out, want_state = run_batch(api, b, mode)
    stream = torch.cuda.Stream()
    t = {k: _dev(torch, b[k]) for k in ("first", "ebits", "sync_id", "rv", "fn", "state")}
    out = torch.zeros(len(b["fn"]) * 80, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    api.tch9_follow_bits_dev(stream.cuda_stream, len(b["calls"]), len(b["fn"]), t["first"].data_ptr(), t["ebits"].data_ptr(),
                             t["sync_id"].data_ptr(), t["rv"].data_ptr(), t["fn"].data_ptr(), t["state"].data_ptr(),
                             out.data_ptr(), mode=mode)
    stream.synchronize()
    assert out.cpu().numpy().tobytes() == want_out.tobytes()
    assert t["state"].cpu().numpy().tobytes() == want_state.tobytes()
    # nothing to do: the device memory stays as it is
    keep, keep_state = out.clone(), t["state"].clone()
    api.tch9_follow_bits_dev(stream.cuda_stream, 0, 0, t["first"].data_ptr(), t["ebits"].data_ptr(), t["sync_id"].data_ptr(), None,
                             t["fn"].data_ptr(), t["state"].data_ptr(), out.data_ptr(), mode=mode)
    stream.synchronize()
    assert torch.equal(keep, out) and torch.equal(keep_state, t["state"])

    # the states after the batch, assigned where they lie: calls 0 and 3, call 0 twice, a negative entry
    call = _dev(torch, np.array([0, -1, 3, 0], np.int32))
    api.tch9_state_assign_batch_dev(stream.cuda_stream, 4, call.data_ptr(), t["state"].data_ptr())
    stream.synchronize()
    host = want_state.copy()
    assert host["n_held"][0] == 2 and host["n_held"][3] == 1
    api.tch9_state_assign(host, index=0)
    api.tch9_state_assign(host, index=3)
    assert t["state"].cpu().numpy().tobytes() == host.tobytes()

    # from samples
    specs = t9.CARRIERS[4]
    cars = [t9.carrier(pkg, orc, *s) for s in specs]
    iq, first, offset, fs, fn = _pack(cars)
    state = np.concatenate([t9.fresh_state(pkg, c["kc"]) for c in cars])
    want_out, want_state = api.tch9_follow(iq, first, offset, fs, fn, state, sps=4)
    s = dict(iq=_dev(torch, iq), first=_dev(torch, first), offset=_dev(torch, offset), fs=_dev(torch, fs), fn=_dev(torch, fn),
             state=_dev(torch, state))
    out = torch.zeros(offset.size * 80, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    api.tch9_follow_dev(stream.cuda_stream, len(cars), offset.size, s["iq"].data_ptr(), s["first"].data_ptr(), s["offset"].data_ptr(),
                        s["fs"].data_ptr(), s["fn"].data_ptr(), s["state"].data_ptr(), out.data_ptr(), sps=4)
    stream.synchronize()
    assert out.cpu().numpy().tobytes() == want_out.tobytes()
    assert s["state"].cpu().numpy().tobytes() == want_state.tobytes()


def test_bad_arguments_leave_everything_alone(gpu_api):
    api = gpu_api
    EINVAL = 22
    a = t9.bits_args(api)
    a["state"]["active"] = 1
    keep_state, keep_out = a["state"].copy(), a["out"].copy()
    good, bad = t9.bits_bad_cases(a)
    dev, host = api._fn("gmr1_hip_tch9_follow_bits_batch_dev"), api._fn("gmr1_hip_tch9_follow_bits_batch")
    order = ("n_calls", "mode", "first", "n_frames", "ebits", "sid", "rv", "fn", "state", "out")
    for change in bad:
        args = [dict(good, **change)[k] for k in order]
        assert host(*args) == -EINVAL, change
        assert dev(None, *args) == -EINVAL, change              # (refused before any pointer is used)
    assert a["state"].tobytes() == keep_state.tobytes() and a["out"].tobytes() == keep_out.tobytes()
    assert host(*[good[k] for k in order]) == 0                 # and the well-formed call runs
    assert (a["out"]["cls"] == t9.TCH9).all() and (a["out"]["type"] == 0x18).all() and a["state"]["n_held"][0] == 2


def test_two_threads_on_two_streams(gpu_api, pkg, orc):
    """Two threads follow different calls at the same time, each on its own stream: they take turns on the device's workspace
    and each gets what it gets alone."""
    import torch
    api = gpu_api
    batches = [t9.batch(pkg, orc, 2), t9.batch(pkg, orc, 1)]
    modes = [2, 1]
    alone = [run_batch(api, b, m) for b, m in zip(batches, modes)]
    tens = [{k: _dev(torch, b[k]) for k in ("first", "ebits", "sync_id", "rv", "fn", "state")} for b in batches]
    outs = [torch.zeros(len(b["fn"]) * 80, dtype=torch.uint8, device="cuda") for b in batches]
    state0 = [t["state"].clone() for t in tens]
    torch.cuda.synchronize()
    errs, done = [], {}
    go = threading.Barrier(2)

    def worker(w):
        try:
            b, t = batches[w], tens[w]
            st = torch.cuda.Stream()
            go.wait()
            for it in range(4):
                with torch.cuda.stream(st):
                    t["state"].copy_(state0[w])
                    outs[w].zero_()
                api.tch9_follow_bits_dev(st.cuda_stream, len(b["calls"]), len(b["fn"]), t["first"].data_ptr(), t["ebits"].data_ptr(),
                                         t["sync_id"].data_ptr(), t["rv"].data_ptr(), t["fn"].data_ptr(), t["state"].data_ptr(),
                                         outs[w].data_ptr(), mode=modes[w])
                st.synchronize()
                assert outs[w].cpu().numpy().tobytes() == alone[w][0].tobytes(), (w, it)
                assert t["state"].cpu().numpy().tobytes() == alone[w][1].tobytes(), (w, it)
            done[w] = True
        except BaseException as e:      # noqa: BLE001 - reported by the main thread
            errs.append((w, repr(e)))

    ts = [threading.Thread(target=worker, args=(w,)) for w in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    assert done.get(0) and done.get(1)
