"""Cases and helpers of tests/test_gpu_rx_voice.py and tests/test_rx_voice_host.py: the calls the audio close-up
(gmr1_hip_tch3_frames_to_audio_dev) is run on with the blocks one oracle decoder per call gives, a numpy restatement of the
close-up rule, the one-shot voice run computed once per capture and Viterbi decoder mode, the push loop of a voice handle,
and the comparison of a run's audio with a fresh oracle decoder per (carrier, chain, call) over the run's own records."""
import numpy as np

import oracle_lib
import rx_stream_tch_cases as cases
import tch3_cases as tc

SPS = cases.SPS
LABEL = dict(arfcn=1000, chain=3, tn=5, call=1)       # call c of the close-up cases: arfcn + c, chain + c, tn + c, call + c


def closeup(first, n_frames, cls):
    """The rule of gmr1_hip_tch3_frames_to_audio_dev restated: first[] clamped as in the follower, a frame whose class is not
    OFF takes the next slot of its call, a call's slots start behind the reporting frames between the first call's first
    frame and its own -> (slot per frame, -1 where it gives none or no call owns it; blocks in front of each call, the last
    entry the number found)"""
    first = [int(v) for v in first]
    n_calls = len(first) - 1
    slot = np.full(n_frames, -1, np.int64)
    base = np.zeros(n_calls + 1, np.int64)
    if n_calls <= 0:
        return slot, base
    rep = np.asarray(cls) != tc.OFF
    clamp = lambda v, lo: min(max(v, lo), n_frames)
    kf = clamp(first[0], 0)
    at = 0
    for c in range(n_calls):
        lo = clamp(first[c], 0)
        hi = clamp(first[c + 1], lo)
        at = int(rep[kf:lo].sum())
        base[c] = at
        for k in range(lo, hi):
            if rep[k]:
                slot[k] = at
                at += 1
    base[n_calls] = at
    return slot, base


def make_calls(api):
    """test_gpu_tch3_voice.make_calls' seven calls with a third of the non-speech frames given class OFF and the others the
    five remaining classes in turn -> its dict plus fn (the frames' own fn, not the records'), label (per call), want (the
    RX_AUDIO blocks: one oracle decoder per call over the reporting frames) and slot (per frame).  Needs no device."""
    import test_gpu_tch3_voice as v
    c = v.make_calls(api)
    rec = c["rec"]
    quiet = np.flatnonzero(rec["type"] != 0x10)
    for j, k in enumerate(quiet):
        rec["cls"][k] = tc.OFF if j % 3 == 0 else (tc.DKAB, tc.DKAB_MISSING, tc.FACCH, tc.ERR, tc.SPEECH)[(j // 3 + j) % 5]
    off = rec["cls"] == tc.OFF
    assert abs(int(off.sum()) - len(quiet) / 3) < 1 and set(rec["cls"][quiet]) == set(range(6))
    first = c["first"]
    n_calls = len(first) - 1
    fn = (np.arange(len(rec), dtype=np.uint32) * 7 + 50000).astype(np.uint32)
    label = np.array([api.tch3_audio_label(LABEL["arfcn"] + q, LABEL["chain"] + q, LABEL["tn"] + q, LABEL["call"] + q)
                      for q in range(n_calls)], np.uint64)
    want = np.zeros(int((~off).sum()), api.RX_AUDIO)
    at = 0
    for q in range(n_calls):
        d = oracle_lib.AmbeDecoder()
        for k in range(first[q], first[q + 1]):
            if rec["cls"][k] == tc.OFF:
                continue
            b = want[at]
            at += 1
            b["arfcn"], b["chain"], b["tn"], b["call"] = (LABEL[f] + q for f in ("arfcn", "chain", "tn", "call"))
            b["cls"], b["fn"] = rec["cls"][k], fn[k]
            if rec["type"][k] == 0x10:
                p, r = d.decode(rec["l2"][k].reshape(2, 10))
                b["pcm"], b["rv"] = p.reshape(320), r
    slot, base = closeup(first, len(rec), rec["cls"])
    assert base[-1] == len(want) and (want["rv"] == -22).any() and want["pcm"].any()
    return dict(c, fn=fn, label=label, want=want, slot=slot, base=base)


def _key(a, arfcn):
    pos = {int(v): i for i, v in enumerate(arfcn)}
    return np.array([pos[int(x)] * 256 + int(c) for x, c in zip(a["arfcn"], a["chain"])], np.int64)


def sorted_by_chain(a, arfcn):
    """stable sort by (carrier, chain)"""
    return a[np.argsort(_key(a, arfcn), kind="stable")] if len(a) else a


_ONE_SHOT = {}


def one_shot(api, name, cap, arfcn):
    """gmr1_hip_rx_run_voice on the whole capture, once per (capture, decoder mode) -> (records, audio, status, chains)"""
    key = (name, api.get_conv_decoder(), bytes(np.asarray(arfcn, np.uint16)))
    if key not in _ONE_SHOT:
        A, n = cap["x"].shape
        offset = np.arange(A, dtype=np.uint64) * np.uint64(n)
        rec, audio, status, chains, found, n_audio = api.rx_run_voice(cap["x"].reshape(-1), cap["t"].reshape(-1), offset,
                                                                      np.full(A, n, np.uint64), sps=SPS, arfcn=arfcn, kc=cap["kc"],
                                                                      max_records=1 << 20, max_audio=1 << 12)
        assert found == len(rec) and n_audio == len(audio)
        rec.setflags(write=False)
        audio.setflags(write=False)
        _ONE_SHOT[key] = (rec, audio, status, chains)
    return _ONE_SHOT[key]


def stream(api, x, t, kc, sizes, arfcn, before_push=None):
    """push (x, t) in pieces of the given sizes (the rest in the last one) through a voice handle
    -> (records, audio, status, n_chains, the audio of each push); before_push(s, xa, ta, last) runs ahead of every push"""
    A, n = x.shape
    rec, audio, at = [], [], 0
    with api.RxStream(A, sps=SPS, arfcn=arfcn, voice=True, kc=kc) as s:
        def push(k, last):
            xa, ta = np.ascontiguousarray(x[:, at:at + k]), np.ascontiguousarray(t[:, at:at + k])
            if before_push:
                before_push(s, xa, ta, last)
            r, a = s.push(xa, tch=ta, last=last)
            rec.append(r.copy())
            audio.append(a.copy())
        for k in sizes:
            k = min(int(k), n - at)
            if at + k >= n:
                break
            push(k, False)
            at += k
        push(n - at, True)
        status, chains, _ = s.status()
    return np.concatenate(rec), np.concatenate(audio), status, chains, audio


def check_audio(api, rec, audio, arfcn, calls_per_carrier=None):
    """A run's audio against its own records: per chain fn strictly increases; the SPEECH blocks match the chain's type-0x10
    records one to one by fn and tn; their samples and verdicts are a fresh oracle decoder's per (carrier, chain, call) over
    those records' l2; every other block is zeros -> (speech blocks, samples that differ, the oracle's samples where ONE
    decoder runs over each whole chain)"""
    n_speech = n_diff = 0
    whole_chain = []
    seen_calls = {}
    for key in sorted(set(_key(audio, arfcn)) | set(_key(rec[rec["type"] == 0x10], arfcn))):
        a = audio[_key(audio, arfcn) == key]
        r = rec[(_key(rec, arfcn) == key) & (rec["type"] == 0x10)]
        assert (np.diff(a["fn"].astype(np.int64)) > 0).all(), "fn does not increase within a chain"
        assert (a["cls"] != tc.OFF).all() and not a["pad"].any() and (a["call"] >= 1).all()
        assert (np.diff(a["call"].astype(np.int64)) >= 0).all()
        sp = a[a["cls"] == tc.SPEECH]
        quiet = a[a["cls"] != tc.SPEECH]
        assert not quiet["pcm"].any() and not quiet["rv"].any()
        assert len(sp) == len(r) and np.array_equal(sp["fn"], r["fn"]) and np.array_equal(sp["tn"], r["tn"])
        seen_calls.setdefault(int(key) // 256, set()).update(int(v) for v in a["call"])
        one = oracle_lib.AmbeDecoder()
        for call in sorted(set(int(v) for v in sp["call"])):
            d = oracle_lib.AmbeDecoder()
            for b, rr in zip(sp[sp["call"] == call], r[sp["call"] == call]):
                p, v = d.decode(rr["l2"][:20].reshape(2, 10))
                n_diff += int((b["pcm"] != p.reshape(320)).sum()) + int((b["rv"] != v).sum())
                whole_chain.append((b["pcm"].copy(), one.decode(rr["l2"][:20].reshape(2, 10))[0].reshape(320)))
        n_speech += len(sp)
    if calls_per_carrier is not None:
        # `call` runs from 1 to the number of assignments on every carrier
        assert seen_calls == {i: set(range(1, m + 1)) for i, m in enumerate(calls_per_carrier)}, seen_calls
    return n_speech, n_diff, whole_chain
