"""AMBE decoder, aimed streams (tests/ambe_aimed.py), without a GPU: what each stream reaches, computed from its frames, and
the CPU oracle against the reference itself on every one of them -- built from its sources where they are, else as
tests/golden/ambe_ref_digests.npz stores its outputs (tests/test_oracle_ambe.py pins that file to the build).

tests/test_gpu_ambe_aimed.py holds the kernel to the oracle on the same streams."""
import ctypes as C

import numpy as np
import pytest

import ambe_aimed as A
import ambe_streams as S
import oracle_lib
import test_oracle_ambe as T

FAMILIES = ("orbit", "histories", "levels", "tones")


@pytest.fixture(scope="module")
def streams():
    return T.aimed_streams()


@pytest.fixture(scope="module")
def cleared(streams):
    """family -> [(pcm, rv) per channel] of the oracle in its `cleared` reading, computed when first asked for"""
    done = {}

    def get(key):
        if key not in done:
            done[key] = T.decode_channels(lambda fr: oracle_lib.ambe_decode(fr, cleared=True), streams[key])
        return done[key]
    return get


def decoder_functions():
    """The decoder's own 2^x, log2 f0 and harmonic count (frame.c:79-130), as the oracle exports them."""
    lib = oracle_lib.lib()
    for n in ("orc_ambe_f0log_sf0", "orc_ambe_f0log_sf1", "orc_ambe_pow2"):
        getattr(lib, n).restype = C.c_float
    return dict(f0log_sf0=lambda b, n, r: lib.orc_ambe_f0log_sf0(C.c_float(b), C.c_float(n), C.c_int(r)),
                f0log_sf1=lambda p: lib.orc_ambe_f0log_sf1(C.c_int(p)),
                pow2=lambda x: lib.orc_ambe_pow2(C.c_float(x)),
                harmonics=lambda f: lib.orc_ambe_harmonics(C.c_float(f)))


def test_orbit_reads_every_row_a_fresh_decoder_can_reach(streams):
    vuv = T.oracle_vuv_table().astype(int)
    chans = streams["orbit"]
    assert len(chans) == 2
    for c, fr in enumerate(chans):
        cov = A.orbit_coverage(fr)
        print("orbit channel %d: %d of %d rows of the period read, %d outside it, %d frames that are not speech"
              % (c, cov["read"], cov["period"], cov["outside"], cov["not_speech"]))
        assert len(fr) >= 5313 and cov["not_speech"] == 0
        assert cov["period"] == 10625 and cov["read"] == 10625 and cov["outside"] == 0
    # channel 0: entry 0 of the codebook, no band voiced, under every pitch; channel 1: some band unvoiced in both subframes
    assert vuv[0] == 0 and set(A.fields_of(chans[0], "vuv")) == {0}
    assert set(A.fields_of(chans[0], "pitch")) == set(range(124))
    used = vuv[A.fields_of(chans[1], "vuv")]
    assert ((used & 0xff) != 0xff).all() and ((used >> 8) != 0xff).all() and len(set(used)) > 20
    # the rows lie all over the table, beyond what fits 16 bits of a signed carry too (synth.c:127-128)
    rows, _ = A.noise_rows(chans[1])
    assert rows.min() < 10 and rows.max() > 53100 and (rows >= 32768).any()


def test_histories_take_every_pitch_transition_and_every_harmonic_count_pair(streams):
    chans = streams["histories"]
    cov = A.histories_coverage(chans, **decoder_functions())
    print("histories: %d channels of %d frames; %d of 61504 (previous pitch, pitch, rule), %d of 124 first-frame pitches, "
          "%d of 2304 (Ls, Ld)" % (len(chans), len(chans[0]), cov["triples"], cov["firsts"], cov["pairs"]))
    assert cov["triples"] == 124 * 124 * 4 == 61504
    assert cov["firsts"] == 124 and cov["first_rules"] == [0]
    assert cov["pairs"] == 48 * 48 == 2304


def test_levels_hold_the_gain_tables_ends(streams, cleared, pkg):
    tab = pkg.api.codec_host_tables()
    gain = tab["gain"].reshape(256, 2)
    assert gain.min() == gain[A.GAIN_QUIET].min() and A.GAIN_LOUD == 255
    assert tab["vuv"][0] == 0 and tab["vuv"][1] == 0xffff
    loud, quiet = A.GAIN_LOUD, A.GAIN_QUIET
    i = np.arange(A.LEVEL_FRAMES)
    want_gain = {"loud": np.full(200, loud), "quiet": np.full(200, quiet), "alt1": np.where(i & 1, quiet, loud),
                 "alt8": np.where((i >> 3) & 1, quiet, loud)}
    assert len(A.level_cases()) == 4 * 3 * 3
    for case, fr, (pcm, rv) in zip(A.level_cases(), streams["levels"], cleared("levels")):
        g, v, p = case.split("-")
        cov = A.levels_coverage(fr)
        assert len(fr) == 200 and np.array_equal(cov["gain"], want_gain[g]), case
        assert cov["vuv"] == {"unvoiced": [0], "voiced": [1]}.get(v, cov["vuv"]) and (v != "anyvuv" or len(cov["vuv"]) > 30), case
        assert cov["pitch"] == {"p0": [0], "p123": [123]}.get(p, cov["pitch"]) and (p != "anypitch" or len(cov["pitch"]) > 60), case
        wrap, peak = A.wrap_fraction(pcm), int(np.abs(pcm.astype(np.int32)).max())
        print("levels %-24s %.2f %% of adjacent-sample steps above 40000, max |pcm| = %d" % (case, 100 * wrap, peak))
        assert not rv.any()
        if g == "loud":
            assert wrap > 0.01, case
        if g == "quiet":
            assert peak < 1000, case


def test_long_tones_take_both_phases_past_1e5_rad(streams):
    fr = streams["tones"][A.TONE_STREAMS.index("long")]
    kinds = ["tone" if (int(f[0]) & 0xfc) == 0xfc else "speech" if S.is_speech(f) else "silence" for f in fr]
    assert kinds == ["tone"] * 1200 + ["speech"] * 50 + ["tone"] * 300
    p = [A.tone_prediction(f) for f in fr[:1200]]
    assert all(q["code"] == 0x8f and q["n"] == 160 and q["freqs"] == (1633, 941) for q in p[:600])
    assert all(q["code"] == 0x7e and q["n"] == 160 and q["freqs"] == (3937, None) for q in p[600:])
    assert (fr[:1200, 1] == 255).all() and (fr[:1200, 0] == 0xff).all()
    ph = A.tone_phases(fr)
    print("long tones: phases after frame 1: %.1f, %.1f; after 600: %.1f, %.1f; after 1200: %.1f, %.1f; at the end: %.1f, %.1f"
          % (*ph[1], *ph[599], *ph[1199], *ph[-1]))
    # glibc's cosf reduces by one multiply below 120 and with 96 bits of 4 / pi above: both, within the first two frames
    assert (ph[1] > 120).all() and 2 * np.pi * 941 / 8000 < 120
    assert ph[599, 0] > 1e5                  # the pair's upper tone alone; its lower one needs the second run
    assert ph[1199, 0] > 4e5 and ph[1199, 1] == ph[599, 1]
    assert (ph[-1] > 1e5).all()
    assert all(c in range(len(fr) + 1) for c in A.TONE_CUTS)


def test_tone_codes_amplitudes_and_votes(streams, cleared):
    named = dict(zip(A.TONE_STREAMS, zip(streams["tones"], cleared("tones"))))
    rejected = {0x7f} | set(range(0xa4, 0xff))
    for a in A.TONE_AMPLS:
        fr, (pcm, rv) = named["codes_a%d" % a]
        cov = A.tones_coverage(fr)
        assert cov["code_sel"] == {(c, s) for c in range(256) for s in range(4)} and cov["ampls"] == {a}
        # a rejected code is -EINVAL wherever a half is selected (tone.c:197-201)
        assert cov["rejected"] == len(rejected) * 3 == 276
        assert {A.tone_code(f)[0] for f, r in zip(fr, cov["rv"]) if r} == rejected
        assert np.array_equal(rv, cov["rv"])
    fr, (pcm, rv) = named["ampl_sweep"]
    cov = A.tones_coverage(fr)
    assert cov["ampls"] == set(range(256)) and cov["codes"] == {A.TONE_SWEEP_CODE} and not rv.any()
    # votes: every bit position decided by exactly four ones where a code has a one, by exactly three where it has a zero
    fr, (pcm, rv) = named["votes"]
    cov = A.tones_coverage(fr)
    assert cov["codes"] == set(A.VOTE_CODES) and not rv.any()
    for b in range(8):
        ones = [c for c in A.VOTE_CODES if (c >> (7 - b)) & 1]
        assert (cov["four"][b] > 0) == bool(ones) and cov["three"][b] > 0, b
    print("votes: frames with exactly four ones per bit position %s, with exactly three %s" % (cov["four"], cov["three"]))
    per_code = {c: np.zeros(8, int) for c in A.VOTE_CODES}
    for f in fr:
        if (int(f[0]) & 0xfc) == 0xfc:
            code, votes = A.tone_code(f)
            per_code[code] += np.where([(code >> (7 - b)) & 1 for b in range(8)], votes == 4, votes == 3)
            assert any(x != code for x in f[2:8])
    assert all((n > 0).all() for n in per_code.values())
    # the oracle hears what the prediction says: the same samples as for six clean copies of the predicted code, silence
    # where nothing is predicted to sound, sound where an amplitude of 3 or more runs at a frequency above 0
    for name, (fr, (pcm, rv)) in named.items():
        again, rv2 = oracle_lib.ambe_decode(A.cleaned(fr), cleared=True)
        assert np.array_equal(again, pcm) and np.array_equal(rv2, rv), name
        for f, out in zip(fr, pcm):
            if (int(f[0]) & 0xfc) != 0xfc:
                continue
            p = A.tone_prediction(f)
            if p["ampl"] < 0.999:
                assert not out.any(), name
            elif p["ampl"] >= 3.0 and p["freqs"][0] > 0:
                assert out.any(), name


@pytest.mark.parametrize("key", FAMILIES)
def test_oracle_against_the_reference_on_the_aimed_streams(streams, cleared, key):
    clean, rv = T.aimed_reference(key)
    got = cleared(key)
    assert np.array_equal(np.concatenate([r for _, r in got]), rv)
    differ, of = T.aimed_differing(key, [p for p, _ in got], clean)
    print("%s: %d of %d %s differ from the reference (%s)" % (
        key, differ, of, "frames" if isinstance(clean, list) or T.AIMED_BLOCK[key] == 1 else "blocks of %d frames" % T.AIMED_BLOCK[key],
        "built here" if isinstance(clean, list) else "stored digests"))
    assert differ == 0
    if key == "tones":
        assert (rv == -22).sum() == 3 * 276 and set(rv.tolist()) == {0, -22}
    else:
        assert not rv.any()
