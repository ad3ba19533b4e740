"""AMBE speech decoder: the CPU oracle (oracle/orc_ambe.c) against the reference itself.

The vocoder is the one part of the reference that compiles from its own sources (libm only), so here the oracle is
PINNED: bit-identical PCM is required against (a) outputs of the reference's program committed under tests/golden/
and (b) the reference built on the spot, on fresh streams -- or, where its sources are absent, that build's outputs on the
same streams as tests/golden/ambe_ref_digests.npz stores them (a 64-bit digest per frame, written by
tests/golden/make_ambe_ref_digests.py and pinned to the build by the last test below wherever the sources are present).

The aimed streams of tests/ambe_aimed.py (tests/test_ambe_aimed_host.py compares the oracle with the reference on them) have
their reference outputs here too: aimed_streams(), aimed_reference()."""
import ctypes as C
import functools
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ambe_aimed as A
import ambe_streams as S
import oracle_lib
import ref_codec

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ambe_vectors.npz")
DIGESTS = os.path.join(os.path.dirname(__file__), "golden", "ambe_ref_digests.npz")
needs_ref = pytest.mark.skipif(not ref_codec.available(), reason="the reference's sources are not on this machine")
SEEDS = [101, 102, 103]


def fresh_streams(seed):
    """The streams the reference is compared on: random, speech-like, mixed (primed)."""
    return [S.primed(fr, seed) for fr in (S.random_stream(1500, seed, speech_only=True), S.speech_like(1500, seed),
                                          S.mixed_stream(1500, seed))]


def rejected_tone_stream():
    return S.mixed_stream(1200, 77, invalid_tones=True)


def frame_digests(pcm):
    """One 64-bit digest per row (a 160-sample pcm frame, or a 10-byte input frame): equal digests = equal rows (what the
    stored reference outputs hold)."""
    return np.array([int.from_bytes(hashlib.blake2b(np.ascontiguousarray(r).tobytes(), digest_size=8).digest(), "little")
                     for r in pcm], np.uint64)


def reference_outputs(key, fr, program=True):
    """The reference's (clean-stack pcm or its digests, rv, program pcm or its digests) for stream `key`: built here when its
    sources are, else as tests/golden/ambe_ref_digests.npz stores them (then the pcm entries are per-frame digests)."""
    if ref_codec.available():
        clean, rv = ref_codec.decode_clean_stack(fr)
        return clean, rv, (ref_codec.decode_with_program(fr) if program else None)
    if not os.path.exists(DIGESTS):
        pytest.skip("neither the reference's sources nor tests/golden/ambe_ref_digests.npz")
    g = np.load(DIGESTS)
    assert np.array_equal(g[key + "_frames_digest"], frame_digests(fr)), "stream changed"
    return g[key + "_clean"], g[key + "_rv"], (g[key + "_pcm"] if program else None)


# ---- the aimed streams: families of channels, every channel a fresh decoder ----

# frames per stored digest of the reference's samples: `histories` is 61 752 frames, stored per block of 16 to keep the file
# small; the digests of the input frames (there to notice a changed generator, not to compare) are per 16 frames throughout
AIMED_BLOCK = {"orbit": 1, "histories": 16, "levels": 1, "tones": 1}
AIMED_FRAMES_BLOCK = 16


def oracle_vuv_table():
    return np.ctypeslib.as_array((C.c_uint16 * 64).in_dll(oracle_lib.lib(), "orc_ambe_vuv")).copy()


@functools.lru_cache(None)
def aimed_streams():
    """family -> its channels, a list of [n, 10] (lengths differ)"""
    lv, tn = A.levels(), A.tones_batch()
    return {"orbit": list(A.orbit(oracle_vuv_table())), "histories": list(A.histories()),
            "levels": [lv[c] for c in A.level_cases()], "tones": [tn[k] for k in A.TONE_STREAMS]}


def decode_channels(decode, chans):
    """[decode(channel) for every channel], each on a decoder of its own; on several threads (the C calls release the
    interpreter lock; one frame first, alone, so that tables built at first use are built once)"""
    decode(chans[0][:1])
    with ThreadPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0))))) as ex:
        return list(ex.map(decode, chans))


def block_digests(chans, block):
    """One 64-bit digest per `block` rows of every channel (a channel's last block may be short; no block spans two
    channels); block = 1 is frame_digests of the channels one after the other."""
    return np.array([int.from_bytes(hashlib.blake2b(np.ascontiguousarray(c[i:i + block]).tobytes(), digest_size=8).digest(), "little")
                     for c in chans for i in range(0, len(c), block)], np.uint64)


_aimed_reference = {}


def aimed_reference(key):
    """The reference entered on a zeroed stack over the channels of family `key` -> (clean, rv [all frames]): clean is the
    list of the channels' pcm where the reference is built here, else the stored digests per AIMED_BLOCK[key] frames."""
    if key not in _aimed_reference:
        chans = aimed_streams()[key]
        if ref_codec.available():
            res = decode_channels(ref_codec.decode_clean_stack, chans)
            _aimed_reference[key] = ([p for p, _ in res], np.concatenate([r for _, r in res]))
        else:
            if not os.path.exists(DIGESTS):
                pytest.skip("neither the reference's sources nor tests/golden/ambe_ref_digests.npz")
            g = np.load(DIGESTS)
            assert np.array_equal(g["aimed_%s_frames_digest" % key], block_digests(chans, AIMED_FRAMES_BLOCK)), "stream changed"
            _aimed_reference[key] = (g["aimed_%s_clean" % key], g["aimed_%s_rv" % key])
    return _aimed_reference[key]


def aimed_differing(key, pcm_chans, clean):
    """How many frames (blocks of frames, where only digests of blocks are known) of the channels' pcm differ from `clean`,
    and of how many."""
    if isinstance(clean, list):
        return sum(int((p != c).any(1).sum()) for p, c in zip(pcm_chans, clean)), sum(len(c) for c in clean)
    return int((block_digests(pcm_chans, AIMED_BLOCK[key]) != clean).sum()), len(clean)


def same_frames(pcm, ref):
    """Per-frame equality of our pcm with the reference's (pcm, or digests where only those are stored)."""
    if ref.dtype == np.uint64:
        return frame_digests(pcm) == ref
    return (pcm == ref).all(1)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name", ["random", "speech", "mixed"])
def test_oracle_matches_reference_program_outputs(gold, name):
    pcm, rv = oracle_lib.ambe_decode(gold[name + "_frames"])
    assert (rv == gold[name + "_rv"]).all()
    assert np.array_equal(pcm, gold[name + "_pcm"])


@pytest.mark.parametrize("name", ["random", "speech", "mixed", "mixed_invalid"])
def test_oracle_cleared_matches_reference_on_clean_stack(gold, name):
    pcm, rv = oracle_lib.ambe_decode(gold[name + "_frames"], cleared=True)
    assert (rv == gold[name + "_rv"]).all()
    assert np.array_equal(pcm, gold[name + "_clean"])
    if name == "mixed_invalid":
        assert (rv != 0).any() and set(rv[rv != 0]) == {-22}       # -EINVAL, src/codec/tone.c:197-201


def test_the_two_readings_of_d9_differ(gold):
    """The uncleared voicing entries matter when a subframe has fewer harmonics than the one before it: often."""
    differ = (gold["speech_pcm"] != gold["speech_clean"]).any(1)
    assert 0 < differ.sum() < len(differ) // 2


def test_unprimed_stream_agrees_with_the_program_once_every_entry_was_written(gold):
    """Without the priming frame the program's first frames show its start-up stack; the oracle starts from zeros.
    After the first frame with 56 harmonics in both subframes the two agree for good."""
    fr = gold["unprimed_frames"]
    pcm, _ = oracle_lib.ambe_decode(fr)
    bad = np.nonzero((pcm != gold["unprimed_pcm"]).any(1))[0]
    assert len(bad) < 20 and (len(bad) == 0 or bad.max() < 60)


def test_unpack_is_the_inverse_of_the_stream_generator():
    rng = np.random.default_rng(3)
    for _ in range(300):
        f = {k: int(rng.integers(0, 1 << w)) for k, w in S.WIDTH.items()}
        got = oracle_lib.ambe_unpack(S.pack(**f))
        want = [f["hoc%d" % (S.ORDER.index(k) - 7)] if k.startswith("hoc") else f[k] for k in S.ORDER]
        assert got == want


def test_silence_dtx_and_short_tone_calls():
    d = oracle_lib.AmbeDecoder()
    pcm, rv = d.decode_frame(S.silence_frame())
    assert rv == 0 and not pcm.any()
    # a tone frame honours N; both halves selected, 1 kHz-ish single tone
    pcm, rv = d.decode_frame(S.tone_frame(0x20, 230, sel=3), N=80)
    assert rv == 0 and pcm[:80].any() and not pcm[80:].any()
    # only the second half
    pcm, rv = oracle_lib.AmbeDecoder().decode_frame(S.tone_frame(0x85, 255, sel=1))
    assert rv == 0 and not pcm[:80].any() and pcm[80:].any()
    # neither half / inactive code
    for fr in (S.tone_frame(0x85, 255, sel=0), S.tone_frame(0xff, 255, sel=3)):
        pcm, rv = oracle_lib.AmbeDecoder().decode_frame(fr)
        assert rv == 0 and not pcm.any()
    out = np.ones(50, np.int16)
    import ctypes as C
    assert oracle_lib.lib().orc_ambe_decode_dtx(d.buf, out.ctypes.data_as(C.c_void_p), C.c_int(50)) == 0
    assert not out.any()


def test_first_frame_with_interpolation_is_defined_here():
    """Decision D10: the reference walks off its arrays on this input; the oracle must neither crash nor poison
    the frames that follow (the oscillator phases keep the odd first step, so the samples differ from a rule-0
    start for good: nothing to compare, only to survive)."""
    fr = S.speech_like(30, 5)
    for rule in (1, 2, 3):
        f = fr.copy()
        f[0, 6] = (f[0, 6] & 0x3f) | (rule << 6)
        pcm, rv = oracle_lib.ambe_decode(f)
        assert (rv == 0).all() and pcm[1:].any()


def test_band_edges_stay_inside_the_spectrum_for_every_reachable_pitch():
    """With a valid pitch history ((L + 1/2) f0 < 1/2) the last band ends at or before bin 64: the product's kernel
    relies on it to leave the 65th bin out."""
    import ctypes as C
    lib = oracle_lib.lib()
    lib.orc_ambe_f0log_sf0.restype = C.c_float
    lib.orc_ambe_f0log_sf1.restype = C.c_float
    worst = 0
    logs = [np.float32(lib.orc_ambe_f0log_sf1(C.c_int(p))) for p in range(128)]
    for before in logs:
        for now in logs:
            for rule in range(4):
                fl = np.float32(lib.orc_ambe_f0log_sf0(C.c_float(before), C.c_float(now), C.c_int(rule)))
                f0 = np.float32(2.0) ** fl
                L = lib.orc_ambe_harmonics(C.c_float(f0))
                w0 = np.float32(f0 * np.float32(2.0 * np.float32(np.pi)))
                edge = int(np.ceil(np.float32(np.float32(np.float32(128.0) / np.float32(2 * np.float32(np.pi))) *
                                              np.float32(L + 0.5)) * w0))
                worst = max(worst, edge)
    assert worst <= 64


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_against_the_reference_built_here(seed):
    for k, fr in enumerate(fresh_streams(seed)):
        pcm, rv = oracle_lib.ambe_decode(fr)
        assert (rv == 0).all()
        # the fully determined comparison: the library entered on a zeroed stack
        clean, rv2, prog = reference_outputs("s%d_%d" % (seed, k), fr)
        assert same_frames(oracle_lib.ambe_decode(fr, cleared=True)[0], clean).all() and (rv2 == 0).all()
        # the program: its uncleared entries are its own stack's, which libc's calls between two frames (stdio
        # refills and flushes) also use - a handful of frames in thousands see an entry that was overwritten
        assert len(prog) == len(fr)
        differ = int((~same_frames(pcm, prog)).sum())
        print("program vs oracle: %d of %d frames differ" % (differ, len(fr)))
        assert differ <= len(fr) // 200


def test_rejected_tone_codes_against_the_reference_built_here():
    fr = rejected_tone_stream()
    clean, rv, _ = reference_outputs("rejected", fr, program=False)
    pcm, rv_o = oracle_lib.ambe_decode(fr, cleared=True)
    assert (rv != 0).any() and np.array_equal(rv, rv_o) and same_frames(pcm, clean).all()


@needs_ref
def test_stored_digests_are_the_reference_built_here():
    """tests/golden/ambe_ref_digests.npz (what the two tests above read where the sources are absent) is this build's."""
    g = np.load(DIGESTS)
    for key, fr, program in [("s%d_%d" % (seed, k), fr, True) for seed in SEEDS for k, fr in enumerate(fresh_streams(seed))] + \
                            [("rejected", rejected_tone_stream(), False)]:
        clean, rv, prog = reference_outputs(key, fr, program)
        assert np.array_equal(g[key + "_clean"], frame_digests(clean)) and np.array_equal(g[key + "_rv"], rv), key
        if program:      # the program's few stack-dependent frames (see above) are allowed to move with the C library
            assert (g[key + "_pcm"] != frame_digests(prog)).sum() <= len(fr) // 200, key
    for key, chans in aimed_streams().items():
        clean, rv = aimed_reference(key)
        assert isinstance(clean, list)
        assert np.array_equal(g["aimed_%s_frames_digest" % key], block_digests(chans, AIMED_FRAMES_BLOCK)), key
        assert np.array_equal(g["aimed_%s_clean" % key], block_digests(clean, AIMED_BLOCK[key])), key
        assert np.array_equal(g["aimed_%s_rv" % key], rv), key
