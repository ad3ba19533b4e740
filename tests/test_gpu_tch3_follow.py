"""The batched TCH3 call follower (gmr1_hip_tch3_follow_batch*) on the GPU against the frame by frame walk of
tests/tch3_cases.py over the CPU oracle's primitives (rx_tch3 and its helpers, reference src/gmr1_rx.c:355-600).

Integer fields of the records and of the state must be equal.  The burst energy is a sum of in_len non-negative float32
terms, which product and restatement add in different orders: they agree within 2 in_len 2^-24 relative, the two running
averages within that plus 4 2^-24 per frame walked (tch3_cases.energy_tol).  Every test first checks on the reference
that all energy decisions of its inputs stay MARGIN away from the threshold, so that bound cannot flip a decision."""
import threading

import numpy as np
import pytest

import tch3_cases as tc

pytestmark = pytest.mark.gpu

SLOT_INTS = ("cls", "type", "len", "ciph", "fn", "conv", "l2", "pad")
STATE_INTS = ("active", "p", "ciph", "weak_cnt", "sync_id", "burst_cnt", "bi_fn", "ebits", "kc")


def _close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= tol * np.abs(want)))


def check_slots(got, want, in_len, what=""):
    assert got.shape == want.shape, what
    for f in SLOT_INTS:
        assert np.array_equal(got[f], want[f]), (what, f, [k for k in range(len(got)) if not np.array_equal(got[f][k], want[f][k])][:8])
    assert _close(got["energy"], want["energy"], tc.energy_tol(in_len)), (what, "energy")


def check_state(got, want, in_len, frames, what=""):
    for f in STATE_INTS:
        assert np.array_equal(got[f], want[f]), (what, f)
    for f in ("energy_dkab", "energy_burst"):
        assert _close(got[f], want[f], tc.energy_tol(in_len, frames)), (what, f, got[f], want[f])


_expected = {}


def expected(pkg, orc, idx, **kw):
    """tc.expected of a whole case, once per Viterbi decoder mode of the oracle; asserts the inputs' margin"""
    key = (idx, int(orc.lib().orc_conv_get_mode()), tuple(sorted((k, bytes(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items())))
    if key not in _expected:
        _expected[key] = tc.expected(pkg, orc, idx, **kw)
        assert min(_expected[key][1]) >= tc.MARGIN, (idx, min(_expected[key][1]))
    return _expected[key]


def run_cases(api, pkg, idxs):
    """One host-form call over the carriers of CASES[idxs] (they share sps) -> (slots per call, states)"""
    cars = [tc.carrier(pkg, i) for i in idxs]
    iq, first, offset, fs, fn = tc.pack(cars)
    state = np.concatenate([tc.initial_state(pkg, c) for c in cars])
    out, state = api.tch3_follow(iq, first, offset, fs, fn, state, sps=cars[0]["sps"])
    return [out[first[i]:first[i + 1]] for i in range(len(cars))], state


def test_five_parameter_sets(gpu_api, pkg, orc, decoder):
    """Every class, a ciphering switch, a call that ends, three oversampling factors, in both Viterbi decoder modes.  An
    invocation has one sps, so the five sets are three host-form invocations: the three sps-4 carriers as three calls of
    one, the sps-2 and the sps-10 carrier one each."""
    seen = set()
    for sps in sorted({c["sps"] for c in tc.CASES}):
        idxs = [i for i, c in enumerate(tc.CASES) if c["sps"] == sps]
        slots, state = run_cases(gpu_api, pkg, idxs)
        for j, i in enumerate(idxs):
            car = tc.carrier(pkg, i)
            want, _, _, want_state = expected(pkg, orc, i)
            check_slots(slots[j], want, car["in_len"], (decoder, i))
            check_state(state[j:j + 1], want_state, car["in_len"], len(want), (decoder, i))
            seen |= set(int(c) for c in slots[j]["cls"])
            # unciphered speech is what was sent
            sent = {s["fn"]: bytes(s["frame0"]) + bytes(s["frame1"]) for s in car["sent"] if s["type"] == "speech"}
            plain = [r for r in slots[j] if r["type"] == 0x10 and not r["ciph"]]
            assert plain and all(bytes(r["l2"]) == sent.get(int(r["fn"])) for r in plain), i
    assert seen == {tc.OFF, tc.DKAB, tc.DKAB_MISSING, tc.FACCH, tc.SPEECH}
    end = run_cases(gpu_api, pkg, [tc.ENDING])[0][0]["cls"].tolist()
    assert end.count(tc.DKAB_MISSING) == 10 and end[-1] == tc.OFF and tc.DKAB_MISSING not in end[end.index(tc.OFF):]


def test_ciphering_switches_on_and_needs_the_key(gpu_api, pkg, orc):
    i = tc.CIPHERED
    car = tc.carrier(pkg, i)
    slots, state = run_cases(gpu_api, pkg, [i])
    slots = slots[0]
    want, _, _, want_state = expected(pkg, orc, i)
    check_slots(slots, want, car["in_len"])
    rec = slots[slots["type"] != 0]
    on = int(np.argmax(rec["ciph"]))
    # ciph goes 0 -> 1 on a FACCH3 message (it only decoded ciphered: the plain attempt comes first), and stays
    assert not rec["ciph"][:on].any() and rec["ciph"][on:].all() and rec["type"][on] == 0x12 and state["ciph"][0] == 1
    sent = {s["fn"]: bytes(s["frame0"]) + bytes(s["frame1"]) for s in car["sent"] if s["type"] == "speech" and s["ciph"]}
    deciphered = [r for r in rec[on:] if r["type"] == 0x10]
    assert deciphered and all(bytes(r["l2"]) == sent[int(r["fn"])] for r in deciphered)
    msgs = {bytes(s["l2"]) for s in car["sent"] if s["type"] == "facch3"}
    assert any(bytes(r["l2"][:10]) in msgs for r in rec[on:] if r["type"] == 0x12)

    # the same carrier with a wrong key: nothing sent after cipher_from comes out, ciphering never switches on.  (A flush of
    # an EMPTY store -- a sync change right behind a flush -- decodes 416 erasures to the all-zero message, whose CRC passes
    # with any key or none: the reference reports it, the oracle walk has it, and so it is the one 0x12 record left.)
    wrong = car["kc"] ^ np.uint8(0xff)
    iq, first, offset, fs, fn = tc.pack([car])
    out, st = gpu_api.tch3_follow(iq, first, offset, fs, fn, tc.initial_state(pkg, car, kc=wrong), sps=car["sps"])
    want_w, _, _, want_state_w = expected(pkg, orc, i, kc=wrong)
    check_slots(out, want_w, car["in_len"], "wrong key")
    check_state(st, want_state_w, car["in_len"], len(out), "wrong key")
    assert st["ciph"][0] == 0 and not out["ciph"].any()
    after = out[(fn >= car["cipher_from_fn"]) & (out["type"] == 0x12)]
    assert not after["l2"].any()
    assert not any(bytes(r["l2"][:10]) in msgs for r in after)
    assert not any(bytes(r["l2"]) == sent.get(int(r["fn"])) for r in out if r["type"] == 0x10)


def test_state_carries_a_call_across_invocations(gpu_api, pkg, orc):
    """A call cut at three places -- in the middle of a four-burst FACCH3 group, twice at the same frame (an empty piece) and
    behind the ciphering switch -- gives, piece by piece with the state passed through host memory, byte for byte the records
    and the final state of the one invocation: it is the same code on the same inputs."""
    i = tc.CIPHERED
    car = tc.carrier(pkg, i)
    _, _, steps, _ = expected(pkg, orc, i)
    mid = next(k + 1 for k in range(len(steps) - 1)
               if steps[k][0] == tc.FACCH and steps[k + 1][0] == tc.FACCH and not steps[k][2] and not steps[k + 1][2])
    n = len(steps)
    cuts = [0, mid, mid, (mid + n) // 2 + 1, n]
    iq, first, offset, fs, fn = tc.pack([car])
    whole, whole_state = gpu_api.tch3_follow(iq, first, offset, fs, fn, tc.initial_state(pkg, car), sps=car["sps"])
    state = tc.initial_state(pkg, car)
    pieces = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out, state = gpu_api.tch3_follow(iq, [0, hi - lo], offset[lo:hi], fs[lo:hi], fn[lo:hi], state, sps=car["sps"])
        if hi == mid and lo < mid:
            assert state["burst_cnt"][0] in (1, 2, 3) and state["ebits"].any()      # the cut lies inside a group
        pieces.append(out)
    assert 0 < mid < n and len(pieces[1]) == 0
    assert np.concatenate(pieces).tobytes() == whole.tobytes()
    assert state.tobytes() == whole_state.tobytes()


def test_grid_shapes(gpu_api, pkg, orc):
    """70 calls of 12 frames (more than one wave per work-group of the walk, more than one work-group; more than one wave of
    the emit step), from three carriers under two (p, key) settings each; a call without frames in the middle; a call whose
    state is all zero; no calls at all."""
    api = gpu_api
    nfr = 12
    cars = [tc.carrier(pkg, i) for i in (0, 1, 2)]
    iq, _, _, _, _ = tc.pack(cars)
    base = np.concatenate([[0], np.cumsum([(c["x"].size + 15) & ~15 for c in cars])])
    rng = np.random.default_rng(77)
    other_kc = rng.integers(0, 256, 8, dtype=np.uint8)
    setting = lambda c, v: dict(p=None, kc=None) if v == 0 else dict(p=(cars[c]["p"] + 9) % 40, kc=other_kc)
    want = {}
    for c in range(3):
        for v in range(2):
            kw = {k: x for k, x in setting(c, v).items() if x is not None}
            sl, mg, _, st = tc.expected(pkg, orc, c, hi=nfr, **kw)
            assert min(mg) >= tc.MARGIN
            want[c, v] = (sl, st)
    calls, first, offset, fs, fn, state = [], [0], [], [], [], []
    sentinel = np.frombuffer(rng.integers(0, 256, api.TCH3_STATE.itemsize, dtype=np.uint8).tobytes(), api.TCH3_STATE).copy()
    for k in range(72):
        if k == 35:                                      # no frames: its state, whatever it holds, stays
            calls.append("empty")
            state.append(sentinel)
            first.append(first[-1])
            continue
        c, v = k % 3, (k // 3) % 2
        if k == 36:                                      # all-zero state: not a call
            calls.append(("off", c))
            state.append(np.zeros(1, api.TCH3_STATE))
        else:
            calls.append((c, v))
            state.append(tc.initial_state(pkg, cars[c], **setting(c, v)))
        offset.append(cars[c]["offset"][:nfr] + np.uint64(base[c]))
        fs.append(cars[c]["freq_shift"][:nfr])
        fn.append(cars[c]["fn"][:nfr])
        first.append(first[-1] + nfr)
    state = np.concatenate(state)
    out, got = api.tch3_follow(iq, first, np.concatenate(offset), np.concatenate(fs), np.concatenate(fn), state, sps=4)
    assert len(out) == 71 * nfr
    il = cars[0]["in_len"]
    for k, what in enumerate(calls):
        sl = out[first[k]:first[k + 1]]
        if what == "empty":
            assert len(sl) == 0 and got[k].tobytes() == sentinel.tobytes()
        elif what[0] == "off":
            assert (sl["cls"] == tc.OFF).all() and not sl["type"].any() and not sl["l2"].any() and not sl["fn"].any()
            assert _close(sl["energy"], want[what[1], 0][0]["energy"], tc.energy_tol(il))
            assert got[k].tobytes() == bytes(api.TCH3_STATE.itemsize)
        else:
            check_slots(sl, want[what][0], il, (k, what))
            check_state(got[k:k + 1], want[what][1], il, nfr, (k, what))
    # no calls: nothing happens, nothing is touched
    none, st = api.tch3_follow(iq, [0], [], [], [], np.zeros(0, api.TCH3_STATE), sps=4)
    assert len(none) == 0 and len(st) == 0


def _dev_inputs(torch, pkg, idxs):
    cars = [tc.carrier(pkg, i) for i in idxs]
    iq, first, offset, fs, fn = tc.pack(cars)
    state = np.concatenate([tc.initial_state(pkg, c) for c in cars])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t = dict(iq=dev(iq), first=dev(first), offset=dev(offset), fs=dev(fs), fn=dev(fn), state=dev(state),
             out=torch.zeros(offset.size * 40, dtype=torch.uint8, device="cuda"))
    return cars, (iq, first, offset, fs, fn, state), t


def _run_dev(api, stream, t, n_calls, n_frames, sps):
    api.tch3_follow_dev(stream.cuda_stream, n_calls, n_frames, t["iq"].data_ptr(), t["first"].data_ptr(), t["offset"].data_ptr(),
                        t["fs"].data_ptr(), t["fn"].data_ptr(), t["state"].data_ptr(), t["out"].data_ptr(), sps=sps)


def test_dev_form_equals_the_host_form(gpu_api, pkg, orc):
    """Everything in device memory, on a stream of the caller's: byte for byte the host form's records and states."""
    import torch
    api = gpu_api
    idxs = [0, 1, 2]
    for i in idxs:
        expected(pkg, orc, i)                            # (margin of the inputs)
    cars, (iq, first, offset, fs, fn, state), t = _dev_inputs(torch, pkg, idxs)
    want_out, want_state = api.tch3_follow(iq, first, offset, fs, fn, state, sps=4)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    _run_dev(api, st, t, len(idxs), offset.size, 4)
    st.synchronize()
    assert t["out"].cpu().numpy().tobytes() == want_out.tobytes()
    assert t["state"].cpu().numpy().tobytes() == want_state.tobytes()
    # nothing to do: the device memory stays as it is
    keep = t["out"].clone()
    api.tch3_follow_dev(st.cuda_stream, 0, 0, t["iq"].data_ptr(), t["first"].data_ptr(), t["offset"].data_ptr(),
                        t["fs"].data_ptr(), t["fn"].data_ptr(), t["state"].data_ptr(), t["out"].data_ptr(), sps=4)
    st.synchronize()
    assert torch.equal(keep, t["out"])


def test_bad_arguments_leave_everything_alone(gpu_api):
    api = gpu_api
    EINVAL = 22
    a = tc.call_args(api)
    a["iq"][:] = np.random.default_rng(5).standard_normal((4096, 2), dtype=np.float32).view(np.complex64).reshape(-1)
    a["state"]["active"] = 1
    keep_state, keep_out = a["state"].copy(), a["out"].copy()
    good, bad = tc.bad_argument_cases(a)
    dev, host = api._fn("gmr1_hip_tch3_follow_batch_dev"), api._fn("gmr1_hip_tch3_follow_batch")
    h = lambda n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out: \
        host(n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out)
    d = lambda n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out: \
        dev(None, n_calls, sps, in_len, iq, first, n_frames, off, fs, fn, state, out)
    for change in bad:
        assert h(**dict(good, **change)) == -EINVAL, change
        assert d(**dict(good, **change)) == -EINVAL, change        # (refused before any pointer is used)
    assert h(**dict(good, iq_len=1473)) == -EINVAL
    for first in ([1, 2], [0, 1], [0, 3]):
        a["first"][:] = first
        assert h(**good) == -EINVAL, first
    a["first"][:] = [0, 2]
    assert a["state"].tobytes() == keep_state.tobytes() and a["out"].tobytes() == keep_out.tobytes()
    assert h(**good) == 0                                # and the well-formed call runs
    assert (a["out"]["cls"] != 0x55).all()


def test_two_threads_on_two_streams(gpu_api, pkg, orc):
    """Two threads follow different calls at the same time, each on its own stream: they take turns on the device's workspace
    and each gets what it gets alone."""
    import torch
    api = gpu_api
    sets = [[0, 2], [1]]
    for i in (0, 1, 2):
        expected(pkg, orc, i)
    inputs = [_dev_inputs(torch, pkg, idxs) for idxs in sets]
    alone = [api.tch3_follow(*h[:5], h[5], sps=4) for _, h, _ in inputs]
    state0 = [t["state"].clone() for _, _, t in inputs]
    torch.cuda.synchronize()
    errs, done = [], {}
    go = threading.Barrier(2)

    def worker(w):
        try:
            _, h, t = inputs[w]
            st = torch.cuda.Stream()
            go.wait()
            for it in range(4):
                with torch.cuda.stream(st):
                    t["state"].copy_(state0[w])
                    t["out"].zero_()
                _run_dev(api, st, t, len(sets[w]), h[2].size, 4)
                st.synchronize()
                assert t["out"].cpu().numpy().tobytes() == alone[w][0].tobytes(), (w, it)
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
