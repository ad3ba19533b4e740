"""Streams of AMBE frames aimed at what the decoder reads -- TEST INFRASTRUCTURE (numpy only, seeded, no oracle, no product).

tests/ambe_streams.py draws frames at random; the decoder's tables and running sums are far larger than what such streams
reach.  Each family here goes after one of them, and comes with a COVERAGE FUNCTION that recomputes, from the frames alone,
what the stream reaches: the tests assert the coverage, nothing is claimed by construction.

    orbit       every row of the noise-spectrum table a fresh decoder can reach (the generator's 80-step walk from 3147)
    histories   every (previous pitch, pitch, interpolation rule) and every first-frame pitch: the fundamental table and,
                through it, every pair of harmonic counts of the regridding table
    levels      the gain table's ends, held and alternating: samples that wrap in the float -> int16 conversion, and tiny ones
    tones       tone phases run far up the float scale, every tone code, every amplitude byte, the majority vote at its edges

Where a coverage function needs the decoder's own numbers (2^x, the harmonic count) the caller hands them in as functions:
this module restates only integer and float32 arithmetic that numpy does exactly."""
from __future__ import annotations

import numpy as np

import ambe_streams as S

N_PITCH = 124                     # pitch values of a speech frame: 124 .. 127 are the silence and tone prefixes
NOISE_START, NOISE_MOD = 3147, 53125        # synth.c:306-311, synth.c:98-110


def speech_frames(rng, n, **fixed):
    """n speech frames [n, 10]: every quantiser index random (pitch below 124), but those named in `fixed` (a value for
    all frames, or one per frame)."""
    f = {k: rng.integers(0, 1 << w, n) for k, w in S.WIDTH.items()}
    f["pitch"] = rng.integers(0, N_PITCH, n)
    for k, v in fixed.items():
        f[k] = np.broadcast_to(np.asarray(v, np.int64), (n,))
    assert (f["pitch"] < N_PITCH).all()
    bits = np.zeros((n, 80), np.uint8)
    for name, parts in S.LAYOUT.items():
        v = f[name].astype(np.int64)
        assert ((0 <= v) & (v < (1 << S.WIDTH[name]))).all(), name
        left = S.WIDTH[name]
        for first, nb in parts:
            left -= nb
            for k in range(nb):
                bits[:, first + k] = (v >> (left + nb - 1 - k)) & 1
    return np.packbits(bits, axis=1)


def rules_after_rule_0(rng, n):
    """Random interpolation rules for a fresh decoder's stream: its first frame takes rule 0 (decision D10)."""
    r = rng.integers(0, 4, n)
    r[:1] = 0
    return r


def fields_of(frames, name):
    """The quantiser index `name` of every frame [n, 10] -> [n] (the inverse of ambe_streams.pack)."""
    bits = np.unpackbits(np.ascontiguousarray(frames, np.uint8).reshape(-1, 10), axis=1).astype(np.int64)
    v = np.zeros(len(bits), np.int64)
    for first, n in S.LAYOUT[name]:
        for k in range(n):
            v = (v << 1) | bits[:, first + k]
    return v


def speech_mask(frames):
    b0 = np.ascontiguousarray(frames, np.uint8).reshape(-1, 10)[:, 0] & 0xfc
    return (b0 != 0xfc) & (b0 != 0xf8)


# ---- orbit: the noise generator's walk ----

ORBIT_FRAMES = 5313               # 10 626 subframes: one more than the walk's period


def lcg(x, steps=1):
    for _ in range(steps):
        x = (x * 171 + 11213) % NOISE_MOD
    return x


def noise_rows(frames, start=NOISE_START):
    """The noise-table row (the generator's state) each subframe of a stream reads [n, 2], -1 where the frame is not speech:
    a speech subframe reads the row of the carried state and carries the state 80 steps on; silence and tone frames step
    nothing.  Returns (rows, the state left behind)."""
    sp = speech_mask(frames)
    rows = np.full((len(sp), 2), -1, np.int64)
    x = start
    for i in np.nonzero(sp)[0]:
        for k in range(2):
            rows[i, k] = x
            x = lcg(x, 80)
    return rows, x


def noise_period(start=NOISE_START):
    """The rows the 80-step walk visits from `start` until it is back there (it is a bijection: it comes back)."""
    seen, x = [], start
    while True:
        seen.append(x)
        x = lcg(x, 80)
        if x == start:
            return np.array(seen, np.int64)


def orbit(vuv_table, n=ORBIT_FRAMES, seed=7000):
    """[2, n, 10]: channel 0 all bands unvoiced in every frame (vuv entry 0), the pitch sweeping 0 .. 123; channel 1 random
    fields with vuv drawn from the entries that leave some band unvoiced in both subframes (neither byte 0xff)."""
    vuv_table = np.asarray(vuv_table).astype(np.int64)
    assert vuv_table.shape == (64,) and vuv_table[0] == 0
    noisy = [i for i, p in enumerate(vuv_table) if (p & 0xff) != 0xff and (p >> 8) != 0xff]
    rng = np.random.default_rng(seed)
    return np.stack([
        speech_frames(rng, n, vuv=0, pitch=np.arange(n) % N_PITCH, pitch_rule=rules_after_rule_0(rng, n)),
        speech_frames(rng, n, vuv=np.asarray(noisy)[rng.integers(0, len(noisy), n)], pitch_rule=rules_after_rule_0(rng, n))])


def orbit_coverage(frames, start=NOISE_START):
    """-> dict(period: rows of the walk's period from `start`, read: distinct rows the stream reads, outside: rows it reads
    that are not in the period, not_speech: frames that step nothing)"""
    rows, _ = noise_rows(frames, start)
    period = set(noise_period(start).tolist())
    read = set(rows[rows >= 0].tolist())
    return dict(period=len(period), read=len(read & period), outside=len(read - period),
                not_speech=int((~speech_mask(frames)).sum()))


# ---- histories: every pitch transition under every rule ----

def _euler_circuit(rng):
    """A closed walk over the pitches that takes every (from, to, rule) once: every pitch has 4 * 124 edges out and as many
    in, so one exists (Hierholzer).  -> [(to, rule)] from pitch 0, 61 504 entries."""
    todo = []
    for a in range(N_PITCH):
        e = [(b, r) for b in range(N_PITCH) for r in range(4)]
        rng.shuffle(e)
        todo.append(e)
    stack, circuit = [(0, -1)], []
    while stack:
        at = stack[-1][0]
        if todo[at]:
            stack.append(todo[at].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()                     # [(0, -1), (p1, r1), ...]: the rule belongs to the step INTO the pitch
    assert circuit[0] == (0, -1) and circuit[-1][0] == 0
    return circuit[1:]


def histories(seed=7100):
    """[124, 498, 10]: channel c opens with pitch c at rule 0 (a decoder's first frame: decision D10), steps to where its
    496-step piece of the closed walk begins, then takes the piece.  Everything but pitch and rule is random."""
    rng = np.random.default_rng(seed)
    walk = _euler_circuit(rng)
    per = len(walk) // N_PITCH
    assert per * N_PITCH == len(walk) == N_PITCH * N_PITCH * 4
    out = np.zeros((N_PITCH, per + 2, 10), np.uint8)
    for c in range(N_PITCH):
        piece = walk[c * per:(c + 1) * per]
        begins = walk[c * per - 1][0]             # where the piece starts from (the walk is closed: -1 is its end, pitch 0)
        steps = [(c, 0), (begins, int(rng.integers(0, 4)))] + piece
        out[c] = speech_frames(rng, len(steps), pitch=[p for p, _ in steps], pitch_rule=[r for _, r in steps])
    return out


def histories_coverage(chans, f0log_sf0, f0log_sf1, pow2, harmonics):
    """chans [n_ch, n, 10], every channel a fresh decoder; the four functions are the decoder's own (frame.c:79-130).
    -> dict(triples: distinct (previous pitch, pitch, rule) of speech frames after a channel's first, firsts: distinct
    pitches of first frames, first_rules: the rules seen there, pairs: distinct (Ls, Ld) the regridding is asked for --
    three a frame: previous frame -> second subframe, previous frame -> first, second -> first)"""
    log1 = [f0log_sf1(p) for p in range(128)]
    L1 = [harmonics(pow2(x)) for x in log1]
    L0 = {}
    triples, firsts, first_rules, pairs = set(), set(), set(), set()
    for fr in chans:
        assert speech_mask(fr).all()
        pitch, rule = fields_of(fr, "pitch"), fields_of(fr, "pitch_rule")
        prev, prev_log, prev_L = 128, 0.0, 30          # ambe.c:43-45: a fresh decoder
        for p, r in zip(pitch.tolist(), rule.tolist()):
            if prev == 128:
                firsts.add(p)
                first_rules.add(r)
            else:
                triples.add((prev, p, r))
            key = (prev, p, r)
            if key not in L0:
                L0[key] = harmonics(pow2(f0log_sf0(prev_log, log1[p], r)))
            pairs.update(((prev_L, L1[p]), (prev_L, L0[key]), (L1[p], L0[key])))
            prev, prev_log, prev_L = p, log1[p], L1[p]
    return dict(triples=len(triples), firsts=len(firsts), first_rules=sorted(first_rules), pairs=len(pairs))


# ---- levels: the ends of the gain table ----

GAIN_LOUD, GAIN_QUIET = 255, 4
LEVEL_FRAMES = 200
LEVEL_GAINS = ("loud", "quiet", "alt1", "alt8")
LEVEL_VUV = ("unvoiced", "voiced", "anyvuv")           # vuv entry 0 (0x0000), entry 1 (0xffff), random
LEVEL_PITCH = ("p0", "p123", "anypitch")


def level_cases():
    return ["%s-%s-%s" % (g, v, p) for g in LEVEL_GAINS for v in LEVEL_VUV for p in LEVEL_PITCH]


def levels(seed=7200):
    """{case: [200, 10]}: the gain index held at 255, held at 4, the two alternating every frame and every 8 frames, each
    with all bands unvoiced / all voiced / random voicing at pitch 0, pitch 123 and random pitches."""
    out = {}
    for n, case in enumerate(level_cases()):
        g, v, p = case.split("-")
        rng = np.random.default_rng(seed + n)
        i = np.arange(LEVEL_FRAMES)
        both = np.array([GAIN_LOUD, GAIN_QUIET])
        fixed = dict(pitch_rule=rules_after_rule_0(rng, LEVEL_FRAMES),
                     gain={"loud": GAIN_LOUD, "quiet": GAIN_QUIET, "alt1": both[i & 1], "alt8": both[(i >> 3) & 1]}[g])
        if v != "anyvuv":
            fixed["vuv"] = 0 if v == "unvoiced" else 1
        if p != "anypitch":
            fixed["pitch"] = 0 if p == "p0" else 123
        out[case] = speech_frames(rng, LEVEL_FRAMES, **fixed)
    return out


def levels_coverage(frames):
    """What the frames of a case hold: the gain indices in order, the distinct vuv and pitch indices."""
    return dict(gain=fields_of(frames, "gain"), vuv=sorted(set(fields_of(frames, "vuv").tolist())),
                pitch=sorted(set(fields_of(frames, "pitch").tolist())))


def wrap_fraction(pcm):
    """The fraction of adjacent-sample steps above 40 000: no signal that fits int16 without wrapping moves that far at
    a rate worth counting."""
    x = np.asarray(pcm, np.int32).reshape(-1)
    return float((np.abs(np.diff(x)) > 40000).mean())


# ---- tones ----

TONE_LONG_CODE, TONE_LONG_SINGLE = 0x8f, 0x7e           # DTMF column 1633 Hz + row 941 Hz; 3 937 Hz
TONE_CUTS = (1, 599, 600, 1201)
VOTE_CODES = (0x85, 0x93, 0x20)
TONE_AMPLS = (255, 119, 0)
TONE_SWEEP_CODE = 0x93


def tone_code(frame):
    """The code a tone frame decodes to: per bit, the majority over its first eight bytes, four of eight being enough
    (tone.c:121-133).  -> (code, votes [8]: ones per bit position, MSB first)"""
    bits = np.unpackbits(np.asarray(frame, np.uint8)[:8].reshape(8, 1), axis=1)
    votes = bits.sum(0)
    code = 0
    for v in votes:
        code = (code << 1) | int(v >= 4)
    return code, votes


def tone_freqs(code):
    """(f1, f2) in Hz, f2 = None for a single tone; None for 0xff (no tone) and for the codes the decoder rejects."""
    k = code & 0xf
    if 0x80 <= code <= 0xa3:
        if code >= 0xa0:
            return ((440, 350), (480, 440), (630, 480), (490, 350))[k]
        if code >= 0x90:
            return (1052, 1162, 1297, 1430)[k >> 2], (606, 672, 743, 820)[k & 3]
        return (1209, 1336, 1477, 1633)[k >> 2], (697, 770, 852, 941)[k & 3]
    if code < 0x7f:
        return (code * 125) >> 2, None
    return None


def tone_prediction(frame, N=160):
    """-> dict(code, votes, rv: the verdict (0 or -22), n: samples the tone runs over, freqs, ampl: the amplitude before
    its conversion to int, halved for a pair of tones (0.0 where nothing sounds))"""
    frame = np.asarray(frame, np.uint8)
    assert (int(frame[0]) & 0xfc) == 0xfc
    code, votes = tone_code(frame)
    sel = int(frame[0]) & 3
    start = 0 if sel & 2 else N >> 1
    stop = N - 1 if sel & 1 else (N >> 1) - 1
    out = dict(code=code, votes=votes, rv=0, n=0, freqs=None, ampl=0.0)
    if start >= stop or code == 0xff:          # neither half selected is looked at before the code is (tone.c:135-150)
        return out
    fq = tone_freqs(code)
    if fq is None:
        out["rv"] = -22
        return out
    ampl = 32767.0 * 2.0 ** ((int(frame[1]) - 255.0) / 17.0)          # tone.c:146
    out.update(n=stop - start + 1, freqs=fq, ampl=ampl / 2 if fq[1] is not None else ampl)
    return out


def tone_phases(frames, N=160):
    """The decoder's two tone phases after each frame [n, 2] float32: running float sums of 2 pi f / 8000 per sample that
    are never wrapped or reset (tone.c:100-114), restated in float32 (numpy's float32 add is the C one)."""
    f32 = np.float32
    two_pi = f32(2.0) * f32(3.141592653589793)
    ph = [f32(0.0), f32(0.0)]
    out = np.zeros((len(frames), 2), np.float32)
    for i, fr in enumerate(frames):
        if (int(fr[0]) & 0xfc) == 0xfc:
            p = tone_prediction(fr, N)
            if p["n"]:
                for k, hz in enumerate(p["freqs"]):
                    if hz is None:
                        continue
                    step = (two_pi * f32(hz)) / f32(8000)
                    # n float32 additions: cumsum over float32 adds left to right in float32
                    ph[k] = np.cumsum(np.concatenate([[ph[k]], np.full(p["n"], step, np.float32)]), dtype=np.float32)[-1]
        out[i] = ph
    return out


def tones_long(seed=7300):
    """One channel: 600 frames of the pair 0x8f at amplitude 255, both halves; 600 frames of the single tone 0x7e; 50 speech
    frames; and 300 more frames of the pair.  The second run of the pair is there because no pair of tones has its lower
    frequency above 941 Hz: 600 frames take that phase to 7.1e4 rad, 900 past 1e5."""
    rng = np.random.default_rng(seed)
    speech = speech_frames(rng, 50, pitch_rule=rules_after_rule_0(rng, 50))
    pair = np.tile(S.tone_frame(TONE_LONG_CODE, 255, 3), (600, 1))
    single = np.tile(S.tone_frame(TONE_LONG_SINGLE, 255, 3), (600, 1))
    return np.concatenate([pair, single, speech, pair[:300]])


def _with_speech(tone_frames, rng, every=7):
    """A speech frame before the first tone frame and after every `every` of them: a tone that touched speech state shows."""
    n_speech = (len(tone_frames) + every - 1) // every + 1
    speech = list(speech_frames(rng, n_speech, pitch_rule=rules_after_rule_0(rng, n_speech)))
    out = []
    for i, t in enumerate(tone_frames):
        if i % every == 0:
            out.append(speech.pop(0))
        out.append(t)
    out.append(speech.pop(0))
    assert not speech
    return np.stack(out)


def tones_codes(seed=7310):
    """{name: [n, 10]}: every code 0x00 .. 0xff under every half selection at the amplitudes of TONE_AMPLS, one channel per
    amplitude, and every amplitude byte for one code; speech frames in between."""
    out = {}
    for k, a in enumerate(TONE_AMPLS):
        rng = np.random.default_rng(seed + k)
        pairs = [(c, s) for c in range(256) for s in range(4)]
        rng.shuffle(pairs)
        out["codes_a%d" % a] = _with_speech([S.tone_frame(c, a, s) for c, s in pairs], rng)
    rng = np.random.default_rng(seed + 9)
    out["ampl_sweep"] = _with_speech([S.tone_frame(TONE_SWEEP_CODE, a, 3) for a in rng.permutation(256)], rng)
    return out


def tones_votes(seed=7320):
    """[n, 10]: for each of VOTE_CODES, frames whose six copies of the code have bits flipped so that a bit position is
    decided by exactly four ones (a one, just) or exactly three (a zero, just) -- the type and amplitude bytes vote too --
    for several amplitude bytes and half selections; in each frame every position is at its edge or, with probability 1/3,
    left clean.  Speech frames in between."""
    rng = np.random.default_rng(seed)
    frames = []
    for code in VOTE_CODES:
        for ampl in (255, 0, 0xaa, 0x55, 200):
            for sel in (3, 1, 2, 0):
                for _ in range(3):
                    f = S.tone_frame(code, ampl, sel)
                    fixed = np.unpackbits(f[:2].reshape(2, 1), axis=1).sum(0)
                    copies = np.unpackbits(f[2:8].reshape(6, 1), axis=1)          # [6, 8], MSB first
                    for b in range(8):
                        if rng.random() < 1.0 / 3.0:
                            continue
                        want = (4 if (code >> (7 - b)) & 1 else 3) - int(fixed[b])
                        col = np.zeros(6, np.uint8)
                        col[rng.permutation(6)[:want]] = 1
                        copies[:, b] = col
                    f[2:8] = np.packbits(copies, axis=1)[:, 0]
                    frames.append(f)
    return _with_speech(frames, rng, every=5)


def cleaned(frames):
    """The stream with every tone frame replaced by six clean copies of the code it is predicted to decode to: a decoder
    that votes as predicted gives the same samples for both."""
    out = np.array(frames, np.uint8)
    for f in out:
        if (int(f[0]) & 0xfc) == 0xfc:
            f[2:8] = tone_code(f)[0]
    return out


def tones_coverage(frames):
    """Over the tone frames of a stream (assumed valid): dict(codes: distinct predicted codes, code_sel: distinct (code,
    half selection), ampls: distinct amplitude bytes, rejected: frames predicted to return -22, four / three: per bit
    position, the frames in which exactly four / exactly three of the eight bytes have a one there, rv: predicted verdicts)"""
    codes, code_sel, ampls = set(), set(), set()
    four, three = np.zeros(8, np.int64), np.zeros(8, np.int64)
    rv = np.zeros(len(frames), np.int32)
    for i, f in enumerate(frames):
        if (int(f[0]) & 0xfc) != 0xfc:
            continue
        p = tone_prediction(f)
        codes.add(p["code"])
        code_sel.add((p["code"], int(f[0]) & 3))
        ampls.add(int(f[1]))
        four += p["votes"] == 4
        three += p["votes"] == 3
        rv[i] = p["rv"]
    return dict(codes=codes, code_sel=code_sel, ampls=ampls, rejected=int((rv != 0).sum()), four=four, three=three, rv=rv)


TONE_STREAMS = ("long", "codes_a255", "codes_a119", "codes_a0", "ampl_sweep", "votes")


def tones_batch():
    """Every tone stream by name, in a fixed order: {"long", "codes_a255", "codes_a119", "codes_a0", "ampl_sweep", "votes"}"""
    out = {"long": tones_long()}
    out.update(tones_codes())
    out["votes"] = tones_votes()
    assert tuple(out) == TONE_STREAMS
    return out


def padded(streams):
    """Streams of unequal length as one [n_ch, n_max, 10] batch, the short ones filled up with silence frames (which change
    nothing in a decoder).  -> (batch, lengths)"""
    n = max(len(s) for s in streams)
    out = np.tile(S.silence_frame(), (len(streams), n, 1))
    for c, s in enumerate(streams):
        out[c, :len(s)] = s
    return out, [len(s) for s in streams]
