"""AMBE speech decoder on the GPU against the oracle on the aimed streams of tests/ambe_aimed.py: every row of the noise table a
fresh decoder can reach, every pitch history and harmonic-count pair, the gain table's ends, long tones, every tone code and
amplitude, the tone vote at its edges.  tests/test_ambe_aimed_host.py asserts what the streams reach and pins the oracle to
the reference on them; here every sample and every verdict of gmr1_hip_codec_decode_batch must equal the oracle's.

Run with -s for the differing-sample counts."""
import numpy as np
import pytest

import ambe_aimed as A
import oracle_lib
import test_oracle_ambe as T

pytestmark = pytest.mark.gpu

FLAGS = ("default", "cleared")


@pytest.fixture(scope="module")
def api(gpu_api):
    return gpu_api


@pytest.fixture(scope="module")
def streams():
    return T.aimed_streams()


@pytest.fixture(scope="module")
def want(streams):
    """(family, "default" | "cleared") -> [(pcm, rv) per channel] of the oracle, computed once when first asked for"""
    done = {}

    def get(key, flags):
        if (key, flags) not in done:
            done[key, flags] = T.decode_channels(lambda fr: oracle_lib.ambe_decode(fr, cleared=flags == "cleared"), streams[key])
        return done[key, flags]
    return get


def decode(api, chans, flags):
    """The channels as one batch of fresh decoders (short ones filled up with silence frames) -> (pcm, rv, state)"""
    batch, _ = A.padded(chans)
    return api.codec_decode_batch(batch, flags=api.CODEC_CLEARED if flags == "cleared" else 0)


def compare(pcm, rv, chans, want, what, where=None):
    """Every channel's samples and verdicts against the oracle's; `where(channel, frame, subframe)` adds to the message
    what the first differing subframe read."""
    differ, total, first = 0, 0, None
    for c, (fr, (wpcm, wrv)) in enumerate(zip(chans, want)):
        n = len(fr)
        assert np.array_equal(rv[c, :n], wrv), "%s: verdicts of channel %d" % (what, c)
        assert not pcm[c, n:].any() and not rv[c, n:].any()          # the silence frames a short channel is filled up with
        bad = pcm[c, :n] != wpcm
        differ += int(bad.sum())
        total += bad.size
        if first is None and bad.any():
            f = int(np.nonzero(bad.any(1))[0][0])
            first = (c, f, 0 if bad[f, :80].any() else 1)
    print("%s: %d of %d samples differ" % (what, differ, total))
    if first is not None:
        msg = "%s: channel %d first differs in frame %d, subframe %d" % ((what,) + first)
        pytest.fail(msg + (where(*first) if where else ""))


@pytest.mark.parametrize("flags", FLAGS)
def test_orbit(api, streams, want, flags):
    chans = streams["orbit"]
    pcm, rv, _ = decode(api, chans, flags)

    def where(c, f, sub):
        return ", which reads row %d of the noise table (u_last)" % A.noise_rows(chans[c])[0][f, sub]
    compare(pcm, rv, chans, want("orbit", flags), "orbit, %s" % flags, where)


def test_orbit_handed_from_the_dense_entry_to_the_call_records(api, streams, want):
    """Channel 1: 4 000 frames through the dense entry, the state it returns handed to gmr1_hip_tch3_frames_to_pcm for the
    next 1 200 frames as 600 speech records with a record of another type after every sixth: k_ambe_calls on rows of the
    noise table that no call from a fresh decoder reaches."""
    fr = streams["orbit"][1]
    wpcm, _ = want("orbit", "default")[1]
    head, n_rec = 4000, 600
    rows, _ = A.noise_rows(fr)
    fresh_reach = set(A.noise_rows(fr[:2 * 700])[0].reshape(-1).tolist())
    assert not fresh_reach & set(rows[head:head + 2 * n_rec].reshape(-1).tolist())
    pcm0, rv0, state = api.codec_decode_batch(fr[None, :head])
    assert np.array_equal(pcm0[0], wpcm[:head]) and not rv0.any()
    rng = np.random.default_rng(7400)
    rec = np.zeros(n_rec + n_rec // 6, api.TCH3_FRAME)
    speech = np.arange(len(rec)) % 7 != 6
    assert speech.sum() == n_rec and (~speech).sum() == 100
    rec["type"][speech], rec["len"][speech] = 0x10, 20
    rec["l2"][speech] = fr[head:head + 2 * n_rec].reshape(n_rec, 20)
    rec["type"][~speech] = np.where(np.arange(100) % 2, 0x12, 0)
    rec["l2"][~speech] = rng.integers(0, 256, (100, 20))
    pcm, rv, state1 = api.tch3_frames_to_pcm(rec, np.array([0, len(rec)], np.int32), state=state)
    assert not rv.any() and not pcm[~speech].any()
    got = pcm[speech].reshape(2 * n_rec, 160)
    differ = int((got != wpcm[head:head + 2 * n_rec]).sum())
    print("orbit, records after %d dense frames: %d of %d samples differ" % (head, differ, got.size))
    assert differ == 0
    # and the decoder is where the dense entry is after the same frames: the other records left it alone
    pcm2, _, state2 = api.codec_decode_batch(fr[None, head:head + 2 * n_rec], state=state)
    assert np.array_equal(pcm2[0], got) and state1.tobytes() == state2.tobytes()


@pytest.mark.parametrize("flags", FLAGS)
def test_histories(api, streams, want, flags):
    """All 124 channels in one batch.  The default flags are the oracle's uncleared reading of decision D9, which
    tests/test_oracle_ambe.py relates to the reference's program; CODEC_CLEARED is the reference on a zeroed stack."""
    chans = streams["histories"]
    pcm, rv, _ = decode(api, chans, flags)
    compare(pcm, rv, chans, want("histories", flags), "histories, %s" % flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_levels(api, streams, want, flags):
    chans = streams["levels"]
    pcm, rv, _ = decode(api, chans, flags)
    compare(pcm, rv, chans, want("levels", flags), "levels, %s" % flags)
    assert np.abs(pcm.astype(np.int32)).max() == 32768           # int16's far end is among the samples


@pytest.mark.parametrize("flags", FLAGS)
def test_tones(api, streams, want, flags):
    chans = streams["tones"]
    pcm, rv, _ = decode(api, chans, flags)
    assert (rv == -22).sum() == 3 * 276
    compare(pcm, rv, chans, want("tones", flags), "tones, %s" % flags)


def test_long_tones_in_pieces_carry_the_phases(api, streams, want):
    fr = streams["tones"][A.TONE_STREAMS.index("long")]
    whole, wrv, wstate = api.codec_decode_batch(fr[None])
    state, parts = None, []
    edges = (0,) + A.TONE_CUTS + (len(fr),)
    for a, b in zip(edges[:-1], edges[1:]):
        p, v, state = api.codec_decode_batch(fr[None, a:b], state=state)
        assert not v.any()
        parts.append(p)
    assert np.array_equal(np.concatenate(parts, axis=1), whole) and state.tobytes() == wstate.tobytes()
    assert np.array_equal(whole[0], want("tones", "default")[A.TONE_STREAMS.index("long")][0])


@pytest.mark.parametrize("N", [80, 160, 400])
def test_reference_style_tone_calls(api, streams, N):
    """gmr1_codec_decode_frame over N samples: the first three frames of the long tone, the phases running on"""
    fr = streams["tones"][A.TONE_STREAMS.index("long")][:3]
    c, d = api.Codec(), oracle_lib.AmbeDecoder()
    try:
        for f in fr:
            audio, rc = c.decode_frame(f, N=N)
            w, wrc = d.decode_frame(f, N=N)
            assert rc == wrc == 0 and audio[:N].any()
            differ = int((audio[:N] != w[:N]).sum())
            print("tone frame over N = %d: %d of %d samples differ" % (N, differ, N))
            assert differ == 0
    finally:
        c.release()
