"""A followed voice call to audio on the GPU: the TCH3 follower's records through the speech decoder's calls instantiation
(gmr1_hip_tch3_frames_to_pcm*: k_ambe_calls) and the follower with the decoder behind it (gmr1_hip_tch3_voice_batch*).

Everything is compared for EQUALITY: the decoder's bar is bit-identical samples (tests/test_gpu_ambe.py), the follower's is
byte-identical records (tests/test_gpu_tch3_follow.py), and nothing here adds arithmetic -- a speech record is two frames
through the decoder the dense entry runs, any other record is what gmr1_codec_decode_dtx writes: zeros, the decoder as it
was."""
import numpy as np
import pytest

import ambe_streams as S
import oracle_lib
import tch3_cases as tc

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 37, 64, 65, 130)          # records per call: none, one, a 64-record step and its neighbours, two steps
GUARD = 64


def _fresh_states(api, n):
    """n decoders as gmr1_hip_codec_init_dev makes them -> (n, codec_state_bytes()) uint8"""
    import torch
    st = torch.zeros((n, api.codec_state_bytes()), dtype=torch.uint8, device="cuda")
    api.codec_init_dev(None, n, st.data_ptr())
    torch.cuda.synchronize()
    return st.cpu().numpy()


def _speech_stream(c, n):
    """n frames for call c: between the calls, tone frames of every family, silence frames and unassigned tone codes occur"""
    kind = (6 - c) % 4
    if kind == 0:
        return S.mixed_stream(n, 4100 + c, invalid_tones=True)
    if kind == 1:
        return S.mixed_stream(n, 4100 + c)
    if kind == 2:
        return S.random_stream(n, 4100 + c)
    return S.speech_like(n, 4100 + c)


def _oracle_audio(rec):
    """One oracle decoder over a call's records: the speech halves in order, 320 zeros / rv 0 at every other record"""
    d = oracle_lib.AmbeDecoder()
    pcm = np.zeros((len(rec), 320), np.int16)
    rv = np.zeros((len(rec), 2), np.int32)
    for k, r in enumerate(rec):
        if r["type"] == 0x10:
            p, v = d.decode(r["l2"].reshape(2, 10))
            pcm[k], rv[k] = p.reshape(320), v
    return pcm, rv


def make_calls(api):
    """The seven calls of SIZES as one record array: dict(first, rec, speech (per call: its speech frames), want_pcm, want_rv).
    Needs no device."""
    rng = np.random.default_rng(4000)
    first = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    rec = np.zeros(first[-1], api.TCH3_FRAME)
    speech = []
    other = 0
    for c, n in enumerate(SIZES):
        is_speech = rng.random(n) >= 1.0 / 3.0
        if n:
            is_speech[int(rng.integers(0, n))] = True            # every call that has records decodes something
        frames = _speech_stream(c, 2 * int(is_speech.sum())) if n else np.zeros((0, 10), np.uint8)
        speech.append(frames)
        at = 0
        for k in range(n):
            r = rec[first[c] + k]
            r["fn"], r["energy"] = 1000 * c + k, rng.random()
            if is_speech[k]:
                r["cls"], r["type"], r["len"] = tc.SPEECH, 0x10, 20
                r["l2"] = frames[at:at + 2].reshape(20)
                at += 2
            else:
                # type 0 and 0x12 under every class value, l2 (and what else the decoder has no business reading) random
                r["cls"], r["type"] = other % 6, (0, 0x12)[(other // 6) % 2]
                r["len"], r["ciph"], r["conv"] = rng.integers(0, 256), rng.integers(0, 2), rng.integers(-99, 99)
                r["l2"], r["pad"] = rng.integers(0, 256, 20), rng.integers(0, 256, 4)
                other += 1
    quiet = rec[rec["type"] != 0x10]
    assert 0.2 < len(quiet) / len(rec) < 0.45
    assert {(int(r["cls"]), int(r["type"])) for r in quiet} == {(c, t) for c in range(6) for t in (0, 0x12)}
    all_speech = np.concatenate(speech)
    assert any(not S.is_speech(f) and f[0] & 0xfc == 0xf8 for f in all_speech) and any(f[0] & 0xfc == 0xfc for f in all_speech)
    want = [_oracle_audio(rec[first[c]:first[c + 1]]) for c in range(len(SIZES))]
    want_pcm, want_rv = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    assert (want_rv == -22).any() and want_pcm.any()                 # an unassigned tone code is among the frames
    return dict(first=first, rec=rec, speech=speech, want_pcm=want_pcm, want_rv=want_rv)


@pytest.fixture(scope="module")
def calls(gpu_api):
    """make_calls plus state0: fresh decoders, but the call without records holds arbitrary bytes (they are never looked at)"""
    c = make_calls(gpu_api)
    state0 = _fresh_states(gpu_api, len(SIZES))
    state0[0] = np.random.default_rng(4001).integers(0, 256, state0.shape[1])
    return dict(c, state0=state0)


@pytest.fixture(scope="module")
def whole(gpu_api, calls):
    """The seven calls in one host-form invocation over guard-filled outputs -> (pcm, rv, states)"""
    api = gpu_api
    n = len(calls["rec"])
    pcm = np.full((n, 320), 0x1357, np.int16)
    rv = np.full((n, 2), 7, np.int32)
    state, _ = api._codec_state(calls["state0"], len(SIZES), 0)       # (a 16-byte aligned copy)
    api._call("gmr1_hip_tch3_frames_to_pcm", len(SIZES), calls["first"].ctypes.data, n, calls["rec"].ctypes.data,
              state.ctypes.data, 0, pcm.ctypes.data, rv.ctypes.data)
    return pcm, rv, state


def _differ(got, want, what):
    n = int((got != want).sum())
    print("%s: %d of %d values differ" % (what, n, want.size))
    return n


def test_records_form_against_the_oracle(gpu_api, calls, whole):
    api = gpu_api
    pcm, rv, state = whole
    assert _differ(rv, calls["want_rv"], "rv") == 0
    assert _differ(pcm, calls["want_pcm"], "pcm") == 0
    quiet = calls["rec"]["type"] != 0x10
    assert not pcm[quiet].any() and not rv[quiet].any()
    # the wrapper gives the same from fresh decoders (the empty call's decoder then is a fresh one)
    pcm2, rv2, state2 = api.tch3_frames_to_pcm(calls["rec"], calls["first"])
    assert np.array_equal(pcm2, pcm) and np.array_equal(rv2, rv) and np.array_equal(state2[1:], state[1:])
    # each call ends where the dense entry ends on its speech halves alone; the call without records keeps its bytes
    for c, frames in enumerate(calls["speech"]):
        if SIZES[c] == 0:
            assert state[c].tobytes() == calls["state0"][c].tobytes()
            assert state2[c].tobytes() == _fresh_states(api, 1)[0].tobytes()
            continue
        _, _, dense = api.codec_decode_batch(frames[None])
        assert state[c].tobytes() == dense[0].tobytes(), c


def _piece(calls, lo, hi):
    first = np.clip(calls["first"] - lo, 0, hi - lo).astype(np.int32)
    return first, calls["rec"][lo:hi]


@pytest.mark.parametrize("cuts", [(50, 200), (3, 41), (104, 104)])
def test_cut_anywhere(gpu_api, calls, whole, cuts):
    """Three invocations, the decoder states carried: (50, 200) cuts two calls mid-way and leaves the first four without a record
    in the middle invocation; (3, 41) leaves all but two there; (104, 104) has an empty middle invocation."""
    api = gpu_api
    n = len(calls["rec"])
    state = calls["state0"].copy()
    pcm, rv = [], []
    edges = (0,) + cuts + (n,)
    for j, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        first, rec = _piece(calls, lo, hi)
        if j == 1:
            assert (np.diff(first) == 0).any()
        p, v, state = api.tch3_frames_to_pcm(rec, first, state=state)
        pcm.append(p)
        rv.append(v)
    assert np.array_equal(np.concatenate(pcm), whole[0]) and np.array_equal(np.concatenate(rv), whole[1])
    assert state.tobytes() == whole[2].tobytes()


def test_device_pointers_a_stream_and_clamping(gpu_api, calls, whole):
    import torch
    api = gpu_api
    n, n_calls = len(calls["rec"]), len(SIZES)
    nb = api.codec_state_bytes()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_rec = dev(calls["rec"])
    wild = calls["first"].copy()
    wild[0], wild[-1] = -5, n + 1000                                  # clamped, the spans still tile 0..n
    st = torch.cuda.Stream()
    for first in (calls["first"], wild):
        d_first = dev(first)
        d_pcm = torch.full((n * 320 + GUARD,), 0x1357, dtype=torch.int16, device="cuda")
        d_rv = torch.full((n * 2 + GUARD,), 7, dtype=torch.int32, device="cuda")
        d_st = torch.cat([dev(calls["state0"]), torch.full((GUARD,), 0x5a, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()
        api.tch3_frames_to_pcm_dev(st.cuda_stream, n_calls, n, d_first.data_ptr(), d_rec.data_ptr(), d_st.data_ptr(),
                                   d_pcm.data_ptr(), d_rv.data_ptr())
        st.synchronize()
        pcm, rv, state = d_pcm.cpu().numpy(), d_rv.cpu().numpy(), d_st.cpu().numpy()
        assert np.array_equal(pcm[:n * 320].reshape(n, 320), whole[0]) and (pcm[n * 320:] == 0x1357).all()
        assert np.array_equal(rv[:n * 2].reshape(n, 2), whole[1]) and (rv[n * 2:] == 7).all()
        assert state[:n_calls * nb].tobytes() == whole[2].tobytes() and (state[n_calls * nb:] == 0x5a).all()
    # rv left out; nothing to do
    d_pcm = torch.zeros((n * 320,), dtype=torch.int16, device="cuda")
    d_st = dev(calls["state0"])
    d_first = dev(calls["first"])
    api.tch3_frames_to_pcm_dev(st.cuda_stream, n_calls, n, d_first.data_ptr(), d_rec.data_ptr(), d_st.data_ptr(), d_pcm.data_ptr())
    api.tch3_frames_to_pcm_dev(st.cuda_stream, 0, 0, d_first.data_ptr(), d_rec.data_ptr(), d_st.data_ptr(), d_pcm.data_ptr())
    st.synchronize()
    assert np.array_equal(d_pcm.cpu().numpy().reshape(n, 320), whole[0])


def test_the_dense_entry_is_what_it_was(gpu_api):
    """The streams of test_gpu_ambe.test_many_channels_against_the_oracle through the dense entry, and all-speech records of
    equal length through the calls entry: the dense entry's samples, verdicts and states."""
    api = gpu_api
    n_ch, n_fr = 96, 150
    fr = np.stack([S.mixed_stream(n_fr, 500 + c, invalid_tones=(c % 5 == 0)) if c % 3 else S.random_stream(n_fr, 500 + c)
                   for c in range(n_ch)])
    pcm, rv, state = api.codec_decode_batch(fr)
    total = 0
    for c in range(n_ch):
        want, wrv = oracle_lib.ambe_decode(fr[c])
        assert (rv[c] == wrv).all()
        total += int((pcm[c] != want).sum())
    print("dense entry: %d of %d samples differ from the oracle" % (total, pcm.size))
    assert total == 0
    rec = np.zeros(n_ch * (n_fr // 2), api.TCH3_FRAME)
    rec["type"], rec["cls"], rec["len"] = 0x10, tc.SPEECH, 20
    rec["l2"] = fr.reshape(-1, 20)
    first = np.arange(n_ch + 1, dtype=np.int32) * (n_fr // 2)
    pcm_c, rv_c, state_c = api.tch3_frames_to_pcm(rec, first)
    assert np.array_equal(pcm_c.reshape(pcm.shape), pcm) and np.array_equal(rv_c.reshape(rv.shape), rv)
    assert state_c.tobytes() == state.tobytes()


# ---- the samples form ----
IDXS = (0, tc.CIPHERED, tc.ENDING)
_want = {}


def _expected(pkg, orc, idx):
    """(tc.expected's records of a whole case, the oracle decoder over them), once per Viterbi decoder mode of the oracle"""
    key = (idx, int(orc.lib().orc_conv_get_mode()))
    if key not in _want:
        slots, margins, _, _ = tc.expected(pkg, orc, idx)
        assert min(margins) >= tc.MARGIN
        _want[key] = (slots,) + _oracle_audio(slots)
    return _want[key]


def _inputs(pkg):
    cars = [tc.carrier(pkg, i) for i in IDXS]
    return cars, tc.pack(cars), np.concatenate([tc.initial_state(pkg, c) for c in cars])


def test_samples_form(gpu_api, pkg, orc, decoder):
    """Three carriers (one ciphered from frame 10 on, one that ends at frame 20) as three calls of one invocation: records and
    call states are the follower's, the audio is the oracle decoder's over the ORACLE's records."""
    api = gpu_api
    cars, (iq, first, offset, fs, fn), state = _inputs(pkg)
    out, st, pcm, rv, cs = api.tch3_voice(iq, first, offset, fs, fn, state, sps=4)
    f_out, f_st = api.tch3_follow(iq, first, offset, fs, fn, state, sps=4)
    assert out.tobytes() == f_out.tobytes() and st.tobytes() == f_st.tobytes()
    for j, i in enumerate(IDXS):
        slots, want_pcm, want_rv = _expected(pkg, orc, i)
        lo, hi = first[j], first[j + 1]
        assert 45 <= hi - lo <= 55 and (slots["type"] == 0x10).sum() >= 3
        assert _differ(rv[lo:hi], want_rv, "rv of case %d (%s)" % (i, decoder)) == 0
        assert _differ(pcm[lo:hi], want_pcm, "pcm of case %d (%s)" % (i, decoder)) == 0
        _, _, dense = api.codec_decode_batch(slots["l2"][slots["type"] == 0x10].reshape(1, -1, 10))
        assert cs[j].tobytes() == dense[0].tobytes()
    j = IDXS.index(tc.ENDING)
    mine = out[first[j]:first[j + 1]]
    active = np.flatnonzero((mine["cls"] != tc.OFF) & (mine["cls"] != tc.DKAB_MISSING))
    assert (mine["cls"] == tc.OFF).any() and active.size and active[-1] < len(mine) - 10
    assert pcm[first[j]:first[j + 1]][:active[-1] + 1].any() and not pcm[first[j]:first[j + 1]][active[-1] + 1:].any()


def test_samples_form_cut_mid_call(gpu_api, pkg, orc):
    """The same carriers as two invocations cut in the middle of every call, both states carried: identical results."""
    api = gpu_api
    cars, (iq, first, offset, fs, fn), state = _inputs(pkg)
    for i in IDXS:
        _expected(pkg, orc, i)                           # (margin of the inputs)
    out, st, pcm, rv, cs = api.tch3_voice(iq, first, offset, fs, fn, state, sps=4)
    cut = [int(first[j]) + (17, 23, 31)[j] for j in range(3)]
    pieces = [[slice(int(first[j]), cut[j]) for j in range(3)], [slice(cut[j], int(first[j + 1])) for j in range(3)]]
    st2, cs2 = state, None
    got = {}
    for sl in pieces:
        idx = np.concatenate([np.arange(s.start, s.stop) for s in sl])
        f2 = np.concatenate([[0], np.cumsum([s.stop - s.start for s in sl])]).astype(np.int32)
        o, st2, p, v, cs2 = api.tch3_voice(iq, f2, offset[idx], fs[idx], fn[idx], st2, codec_state=cs2, sps=4)
        for k, a, b, c in zip(idx, o, p, v):
            got[int(k)] = (a.tobytes(), b.tobytes(), c.tobytes())
    assert sorted(got) == list(range(len(out)))
    assert all(got[k] == (out[k].tobytes(), pcm[k].tobytes(), rv[k].tobytes()) for k in range(len(out)))
    assert st2.tobytes() == st.tobytes() and cs2.tobytes() == cs.tobytes()


def test_samples_form_on_device_pointers(gpu_api, pkg, orc):
    """Everything in device memory on a stream of the caller's: byte for byte the host form."""
    import torch
    api = gpu_api
    cars, (iq, first, offset, fs, fn), state = _inputs(pkg)
    for i in IDXS:
        _expected(pkg, orc, i)
    out, st, pcm, rv, cs = api.tch3_voice(iq, first, offset, fs, fn, state, sps=4)
    n, n_calls = offset.size, len(IDXS)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t = [dev(a) for a in (iq, first, offset, fs, fn, state)]
    d_out = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    d_cs = torch.zeros((n_calls, api.codec_state_bytes()), dtype=torch.uint8, device="cuda")
    d_pcm = torch.full((n * 320 + GUARD,), 0x1357, dtype=torch.int16, device="cuda")
    d_rv = torch.full((n * 2 + GUARD,), 7, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.codec_init_dev(s.cuda_stream, n_calls, d_cs.data_ptr())
    api.tch3_voice_dev(s.cuda_stream, n_calls, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                       t[5].data_ptr(), d_out.data_ptr(), d_cs.data_ptr(), d_pcm.data_ptr(), d_rv.data_ptr(), sps=4)
    s.synchronize()
    assert d_out.cpu().numpy().tobytes() == out.tobytes() and t[5].cpu().numpy().tobytes() == st.tobytes()
    assert d_cs.cpu().numpy().tobytes() == cs.tobytes()
    got_pcm, got_rv = d_pcm.cpu().numpy(), d_rv.cpu().numpy()
    assert np.array_equal(got_pcm[:n * 320].reshape(n, 320), pcm) and (got_pcm[n * 320:] == 0x1357).all()
    assert np.array_equal(got_rv[:n * 2].reshape(n, 2), rv) and (got_rv[n * 2:] == 7).all()
