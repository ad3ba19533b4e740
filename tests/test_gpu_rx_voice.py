"""Voice calls to audio in the receive loop on the GPU: the close-up of the TCH3 follower's frames into audio blocks with the
decoder's audio instantiation behind it (gmr1_hip_tch3_frames_to_audio_dev: k_tch3f_audio, k_ambe_audio), fresh decoders
for a list of calls (gmr1_hip_codec_init_list_dev), the one-shot loop (gmr1_hip_rx_run_voice*) and the streaming handle
(gmr1_hip_rx_stream_create_voice / _push_voice*).

Everything is compared for EQUALITY, every block: the decoder's bar is bit-identical samples (tests/test_gpu_ambe.py), the
loop's is byte-identical records (tests/test_gpu_rx_stream_tch.py), and nothing here adds arithmetic."""
import ctypes as C

import numpy as np
import pytest

import rx_stream_tch_cases as cases
import rx_voice_cases as vc
import tch3_cases as tc
import test_gpu_rx_stream as plain
import test_gpu_tch3_voice as v

pytestmark = pytest.mark.gpu

SPS = cases.SPS
GUARD = 4                       # blocks behind the ones a call may write


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if not a.size:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")        # (an array without elements still has an address)
    return torch.from_numpy(a.copy()).cuda()


@pytest.fixture(scope="module")
def calls(gpu_api):
    """rx_voice_cases.make_calls plus state0 (fresh decoders, arbitrary bytes for the call without frames) and what
    gmr1_hip_tch3_frames_to_pcm_dev leaves of it on the same frames"""
    import torch
    api = gpu_api
    c = vc.make_calls(api)
    state0 = v._fresh_states(api, len(v.SIZES))
    state0[0] = np.random.default_rng(4001).integers(0, 256, state0.shape[1])
    n = len(c["rec"])
    d_st, d_pcm = _dev(state0), torch.zeros(n * 320, dtype=torch.int16, device="cuda")
    d_first, d_rec = _dev(c["first"]), _dev(c["rec"])
    torch.cuda.synchronize()
    api.tch3_frames_to_pcm_dev(None, len(v.SIZES), n, d_first.data_ptr(), d_rec.data_ptr(), d_st.data_ptr(), d_pcm.data_ptr())
    torch.cuda.synchronize()
    return dict(c, state0=state0, pcm_states=d_st.cpu().numpy().reshape(state0.shape))


def _close_up(api, c, first, rec, fn, state, max_out, stream=None):
    """one invocation on device copies -> (the blocks with GUARD more behind them, n_out, the states)"""
    import torch
    n_calls = len(first) - 1
    d_first, d_rec, d_fn, d_label, d_st = _dev(first), _dev(rec), _dev(fn), _dev(c["label"]), _dev(state)
    d_out = torch.full(((max_out + GUARD) * 656,), 0x5a, dtype=torch.uint8, device="cuda")
    d_n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    api.tch3_frames_to_audio_dev(stream, n_calls, len(rec), d_first.data_ptr(), d_rec.data_ptr(), d_fn.data_ptr(), d_label.data_ptr(),
                                 d_st.data_ptr(), d_out.data_ptr(), max_out, d_n.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(api.RX_AUDIO), int(d_n.cpu()[0]), d_st.cpu().numpy().reshape(state.shape)


def _same_blocks(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    bad = [k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes()]
    print("%s: %d of %d blocks differ" % (what, len(bad), len(want)))
    assert not bad, (what, bad[:5])


def test_close_up_against_the_oracle(gpu_api, calls):
    import torch
    api = gpu_api
    c = calls
    want, n = c["want"], len(c["rec"])
    assert (c["rec"]["cls"] == tc.OFF).any() and len(want) < n
    st = torch.cuda.Stream()
    got, n_out, state = _close_up(api, c, c["first"], c["rec"], c["fn"], c["state0"], n, st.cuda_stream)
    assert n_out == len(want)
    _same_blocks(got[:n_out], want, "blocks")
    assert (got[n_out:].view(np.uint8) == 0x5a).all()
    # the decoders end where gmr1_hip_tch3_frames_to_pcm_dev leaves them; the call without frames keeps its bytes
    assert state.tobytes() == c["pcm_states"].tobytes()
    assert state[0].tobytes() == c["state0"][0].tobytes()
    # first[] outside 0..n_frames is clamped
    wild = c["first"].copy()
    wild[0], wild[-1] = -5, n + 1000
    got2, n2, state2 = _close_up(api, c, wild, c["rec"], c["fn"], c["state0"], n)
    assert n2 == n_out and got2.tobytes() == got.tobytes() and state2.tobytes() == state.tobytes()
    # nothing to do
    d_n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    api.tch3_frames_to_audio_dev(None, 0, 0, 16, 16, 16, 16, 16, None, 0, d_n.data_ptr())
    torch.cuda.synchronize()
    assert int(d_n.cpu()[0]) == 0


@pytest.mark.parametrize("cuts", [(50, 200), (3, 41), (104, 104)])
def test_close_up_cut_anywhere(gpu_api, calls, cuts):
    """Three invocations, the decoder states carried (the cuts of test_gpu_tch3_voice.test_cut_anywhere)"""
    api = gpu_api
    c = calls
    n = len(c["rec"])
    state = c["state0"]
    blocks = []
    edges = (0,) + cuts + (n,)
    for lo, hi in zip(edges[:-1], edges[1:]):
        first = np.clip(c["first"] - lo, 0, hi - lo).astype(np.int32)
        got, n_out, state = _close_up(api, c, first, c["rec"][lo:hi], c["fn"][lo:hi], state, hi - lo)
        assert n_out == int((c["rec"]["cls"][lo:hi] != tc.OFF).sum())
        blocks.append(got[:n_out])
    _same_blocks(np.concatenate(blocks), c["want"], "blocks of three invocations")
    assert state.tobytes() == c["pcm_states"].tobytes()


def test_close_up_stores_the_first_max_out_blocks_and_decodes_them_all(gpu_api, calls):
    api = gpu_api
    c = calls
    max_out = 70
    base = c["base"]
    inside = [q for q in range(len(v.SIZES)) if base[q] < max_out < base[q + 1]]
    assert inside and v.SIZES[inside[0]] >= 64                   # the cap falls inside a call of more than one step's worth
    got, n_out, state = _close_up(api, c, c["first"], c["rec"], c["fn"], c["state0"], max_out)
    assert n_out == len(c["want"])
    _same_blocks(got[:max_out], c["want"][:max_out], "stored prefix")
    assert (got[max_out:].view(np.uint8) == 0x5a).all()
    assert state.tobytes() == c["pcm_states"].tobytes()
    # nothing stored at all
    got0, n0, state0 = _close_up(api, c, c["first"], c["rec"], c["fn"], c["state0"], 0)
    assert n0 == n_out and (got0.view(np.uint8) == 0x5a).all() and state0.tobytes() == state.tobytes()


def test_init_list_makes_the_listed_decoders_fresh(gpu_api):
    import torch
    api = gpu_api
    nb = api.codec_state_bytes()
    rng = np.random.default_rng(99)
    state = rng.integers(0, 256, (40, nb), dtype=np.uint8)
    call = np.array([3, -1, 17, 3, 39, 0, -5, 17, 22], np.int32)
    fresh = v._fresh_states(api, 1)[0]
    d_state, d_call = _dev(state), _dev(call)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.codec_init_list_dev(st.cuda_stream, call.size, d_call.data_ptr(), d_state.data_ptr())
    api.codec_init_list_dev(st.cuda_stream, 0, d_call.data_ptr(), d_state.data_ptr())
    st.synchronize()
    got = d_state.cpu().numpy().reshape(40, nb)
    named = set(int(x) for x in call if x >= 0)
    for k in range(40):
        assert got[k].tobytes() == (fresh if k in named else state[k]).tobytes(), k
    # GMR1_HIP_CODEC_CLEARED reaches the states as it does through gmr1_hip_codec_init_dev
    d2 = _dev(state)
    api.codec_init_list_dev(None, 1, d_call.data_ptr(), d2.data_ptr(), api.CODEC_CLEARED)
    d3 = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    api.codec_init_dev(None, 1, d3.data_ptr(), api.CODEC_CLEARED)
    torch.cuda.synchronize()
    assert d2.cpu().numpy().reshape(40, nb)[3].tobytes() == d3.cpu().numpy().tobytes() != fresh.tobytes()


# ---- the loops ----
def _check_one_shot(api, name, cap, arfcn, calls_per_carrier=None):
    rec, audio, status, chains = vc.one_shot(api, name, cap, arfcn)
    ref, rst, rch = cases.one_shot(api, name, cap, arfcn)
    assert rec.tobytes() == ref.tobytes() and np.array_equal(status, rst) and np.array_equal(chains, rch)
    key = vc._key(audio, arfcn)
    assert (np.diff(key) >= 0).all(), "blocks do not come by carrier, chain"
    n_speech, n_diff, whole_chain = vc.check_audio(api, rec, audio, arfcn, calls_per_carrier)
    print("%s: %d blocks, %d of speech, %d values differ from the oracle" % (name, len(audio), n_speech, n_diff))
    assert n_speech > 0 and n_diff == 0
    assert audio["pcm"].any()
    return rec, audio, whole_chain


def test_one_shot_on_pairs(gpu_api, pkg, orc, decoder):
    api = gpu_api
    cap = cases.pairs(pkg)
    arfcn = np.arange(cap["x"].shape[0], dtype=np.uint16) + 200
    rec, audio, _ = _check_one_shot(api, "pairs", cap, arfcn)
    assert (audio["call"] == 1).all()
    noise = audio[audio["arfcn"] == arfcn[-1]]
    assert not (noise["cls"] == tc.SPEECH).any() and not noise["pcm"].any()
    assert len(set(audio[audio["cls"] == tc.SPEECH]["arfcn"])) >= 4
    # max_audio below the number found: the first blocks, the count unchanged; no traffic carrier: gmr1_hip_rx_run's records
    A, n = cap["x"].shape
    offset, length = np.arange(A, dtype=np.uint64) * np.uint64(n), np.full(A, n, np.uint64)
    rec2, audio2, _, _, found, n_audio = api.rx_run_voice(cap["x"].reshape(-1), cap["t"].reshape(-1), offset, length, sps=SPS,
                                                          arfcn=arfcn, kc=cap["kc"], max_records=1 << 20, max_audio=33)
    assert n_audio == len(audio) > 33 and audio2.tobytes() == audio[:33].tobytes() and rec2.tobytes() == rec.tobytes()
    rec3, audio3, status3, chains3, _, n3 = api.rx_run_voice(cap["x"].reshape(-1), None, offset, length, sps=SPS, arfcn=arfcn,
                                                             max_records=1 << 20)
    plain_rec, pst, pch, _ = api.rx_run(cap["x"].reshape(-1), offset, length, sps=SPS, arfcn=arfcn, max_records=1 << 20)
    assert n3 == 0 and len(audio3) == 0 and rec3.tobytes() == plain_rec.tobytes()
    assert np.array_equal(status3, pst) and np.array_equal(chains3, pch)


def test_one_shot_on_reassigned(gpu_api, pkg, orc, decoder):
    """Chains assigned twice and three times: a fresh decoder at every assignment, and the blocks of several invocations
    handed back chain by chain"""
    api = gpu_api
    cap = cases.reassigned(pkg)
    arfcn = np.array([0, 1], np.uint16)
    _, audio, whole_chain = _check_one_shot(api, "reassigned", cap, arfcn, calls_per_carrier=[len(ia) for ia in cap["ia"]])
    # the capture tests the reset: ONE decoder over a whole chain gives other samples somewhere
    assert any((got != one).any() for got, one in whole_chain)


def _check_stream(api, name, cap, arfcn, sizes, **kw):
    ref_rec, ref_audio, rst, rch = vc.one_shot(api, name, cap, arfcn)
    rec, audio, status, chains, pushes = vc.stream(api, cap["x"], cap["t"], cap["kc"], sizes, arfcn, **kw)
    assert np.array_equal(status, rst) and np.array_equal(chains, rch)
    assert plain._sorted(rec, arfcn).tobytes() == ref_rec.tobytes(), "streamed records differ from the one-shot call's"
    _same_blocks(vc.sorted_by_chain(audio, arfcn), ref_audio, "streamed audio (%s)" % name)
    for p in pushes:
        assert (np.diff(vc._key(p, arfcn)) >= 0).all()
    return pushes


@pytest.mark.timeout(600)
@pytest.mark.parametrize("sched", ["one", "10ms", "random"])
def test_stream_on_pairs(gpu_api, pkg, decoder, sched):
    """test_gpu_rx_stream's schedules: "random" has pushes shorter than a frame and zero-length pushes"""
    cap = cases.pairs(pkg)
    arfcn = np.arange(cap["x"].shape[0], dtype=np.uint16) + 200
    sizes = plain._schedule(sched, cap["x"].shape[1])
    if sched == "random":
        assert 0 in sizes and any(0 < s < 24 * 39 * SPS for s in sizes)
    pushes = _check_stream(gpu_api, "pairs", cap, arfcn, sizes)
    if sched != "one":
        assert sum(bool(len(p)) for p in pushes) >= 2, "audio should come out as the call goes on"


@pytest.mark.timeout(600)
@pytest.mark.parametrize("sched", ["one", "10ms", "random"])
def test_stream_on_reassigned(gpu_api, pkg, decoder, sched):
    cap = cases.reassigned(pkg)
    arfcn = np.array([0, 1], np.uint16)
    _check_stream(gpu_api, "reassigned", cap, arfcn, plain._schedule(sched, cap["x"].shape[1]))


@pytest.mark.timeout(300)
def test_stream_on_device_pointers_with_a_stride(gpu_api, pkg):
    """_push_voice_dev on a caller's stream, the carriers iq_stride > n apart"""
    import torch
    api = gpu_api
    cap = cases.reassigned(pkg)
    arfcn = np.array([0, 1], np.uint16)
    ref_rec, ref_audio, rst, rch = vc.one_shot(api, "reassigned", cap, arfcn)
    A, n = cap["x"].shape
    step, stride = 50000, 50000 + 24
    pad = lambda a: np.concatenate([a, np.full((A, stride - a.shape[1]), 7 + 7j, np.complex64)], axis=1)
    st = torch.cuda.Stream()
    rec, audio = [], []
    with api.RxStream(A, sps=SPS, arfcn=arfcn, voice=True, kc=cap["kc"]) as s:
        for at in range(0, n, step):
            k = min(step, n - at)
            d_x, d_t = _dev(pad(cap["x"][:, at:at + k])), _dev(pad(cap["t"][:, at:at + k]))
            torch.cuda.synchronize()
            r, a = s.push_dev(st.cuda_stream, d_x.data_ptr(), stride, k, last=at + k >= n, tch_ptr=d_t.data_ptr())
            rec.append(r.copy())
            audio.append(a.copy())
        status, chains, _ = s.status()
    assert np.array_equal(status, rst) and np.array_equal(chains, rch)
    assert plain._sorted(np.concatenate(rec), arfcn).tobytes() == ref_rec.tobytes()
    _same_blocks(vc.sorted_by_chain(np.concatenate(audio), arfcn), ref_audio, "streamed audio, device pointers")


@pytest.mark.timeout(300)
def test_stream_refusals_leave_the_handle_unchanged(gpu_api, pkg):
    api = gpu_api
    cap = cases.reassigned(pkg)
    arfcn = np.array([0, 1], np.uint16)
    A, n = cap["x"].shape
    push_tch, push_voice = api._fn("gmr1_hip_rx_stream_push_tch"), api._fn("gmr1_hip_rx_stream_push_voice")
    push, push_full = api._fn("gmr1_hip_rx_stream_push"), api._fn("gmr1_hip_rx_stream_push_full")
    got_n, got_a = C.c_int(7), C.c_int(7)
    refused = []

    with api.RxStream(A, sps=SPS, arfcn=arfcn, tch=True, kc=cap["kc"]) as s_tch:
        def before_push(s, xa, ta, last):
            k = xa.shape[1]
            m, ma = s.max_records(k), s.max_audio(k)
            assert ma > 0 and s_tch.max_audio(k) == 0
            out, audio = np.empty(max(m, 1), api.RX_RECORD), np.empty(ma, api.RX_AUDIO)
            x, t, o, a = xa.ctypes.data, ta.ctypes.data, out.ctypes.data, audio.ctypes.data
            # the other kinds' entries on a voice handle, the voice entry on a tch handle
            assert push(s._h, x, k, k, 0, o, out.size, C.byref(got_n)) == -22
            assert push_tch(s._h, x, t, k, k, 0, o, out.size, C.byref(got_n)) == -22 and got_n.value == 0
            assert push_full(s._h, x, t, t, k, k, 0, o, out.size, C.byref(got_n), None, 0, C.byref(got_a)) == -22
            assert push_voice(s_tch._h, x, t, k, k, 0, o, out.size, C.byref(got_n), a, ma, C.byref(got_a)) == -22
            # a block buffer one below the bound, none at all, no count, no traffic samples
            assert push_voice(s._h, x, t, k, k, 0, o, out.size, C.byref(got_n), a, ma - 1, C.byref(got_a)) == -22
            assert got_n.value == 0 and got_a.value == 0
            assert push_voice(s._h, x, t, k, k, 0, o, out.size, C.byref(got_n), None, ma, C.byref(got_a)) == -22
            assert push_voice(s._h, x, t, k, k, 0, o, out.size, C.byref(got_n), a, ma, None) == -22
            if k:
                assert push_voice(s._h, x, None, k, k, 0, o, out.size, C.byref(got_n), a, ma, C.byref(got_a)) == -22
            with pytest.raises(ValueError):
                s.push(xa)
            refused.append(k)

        _check_stream(api, "reassigned", cap, arfcn, [60000] * (n // 60000 + 1), before_push=before_push)
    assert len(refused) >= 5
