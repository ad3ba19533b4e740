"""The K=9 (k_xch), K=7 (k_tch3 / tch3_body.h) and K=5-family (k_facch3, k_nt9 for FACCH9 and the three TCH9 modes, k_rach)
Viterbi decoders against the oracle on the pool of tests/decoder_patterns.py: constants, saturated codewords, every single
flipped position of a burst, blocks far from every codeword, all of it again under a cipher stream where the channel has
one.  Every output of every block must equal the oracle's, in both decoder modes (tests/test_decoder_patterns_host.py
checks, without a GPU, that the patterns are what they claim).

What the patterns aim at is integer and exact, and random data almost never goes there.  The figures below are DERIVED FROM
THE CODE, not measured:

  * k_xch keeps [metric:16 | window decisions:16] words; the metric half is 2*ae - sum(K) + kBias with kBias = 0x6000 =
    24576, and the minimum is set back to kBias after every fourth 16-step window and between the two passes.  A soft bit v
    costs ((v -+ 127)^2) >> 9 against a coded 0 / 1: 0 and 126 for +127, 127 and 0 for -128, so K = cost(0) + cost(1) is at
    most 127 a sent bit, and since ae >= 0 the minimum falls by at most 127 a sent bit between two renormalisations,
    whatever the input.  A step has three coded bits, 3 * 127 = 381, and 64 * 381 = 24384 would leave 192; but P(12;13)
    sends 27 of every 39 (two bits a step, three in every thirteenth), at most 133 in 64 steps: 133 * 127 = 16891, which
    leaves 7685.  A codeword of all coded ones sent as -128 takes all of it; 'cw drift' is that form of a random payload
    (about 16 800), 'cw +-127' moves 126 a bit.  So a bias down to 16891 is safe and one below is not: with kBias = 0x4000
    (16384) this file fails on 'cw +-127', and the random-data tests of test_gpu_xch.py still pass; with 0x5000 nothing can.
    Upwards the unreachable states start at 0xF000 and every state is reached after K - 1 = 8 steps, in which a word rises
    by at most 8 * 381 = 3048 < 0x0FFF; afterwards no word is more than 8 * 2 * 381 = 6096 above the minimum.
  * tch3_body.h (K=7 tail-biting, 48 steps, 12-step windows, a warm-up pass on packed u16 metrics) keeps the same form with
    kBias = 0x4000 = 16384 and never renormalises inside a pass; the minimum is set back to kBias between the two.  P(1;2)
    sends three of every four coded bits, 72 a pass: the minimum falls by at most 72 * 127 = 9144, which leaves 7240 (ACC:
    |in| costs, at most 256 a step, 12288 over 48 steps either way).  Unreachable states: 0xF000 + 6 * 254 < 0xFFFF.
  * k_facch3 / k_nt9 / k_rach keep plain costs from zero upwards, unreachable states at 0xF000 = 61440: their edge is the
    opposite one, saturated soft bits far from every codeword.  A step costs at most 127 N.  k_facch3 (N = 4, 96 steps)
    never renormalises: 96 * 508 = 48768, plus a spread of K - 1 = 4 steps (2032), stays below 61440, and a flushed state's
    0xF000 + 2032 below 65536.  k_nt9 / k_rach take the row minimum off after every fourth 16-step window, first after
    4 + 64 steps: at N = 5 (TCH9 2k4) 68 * 635 + 4 * 635 = 45720 < 61440 and 61440 + 2540 < 65536.  These are bounds on any
    input; the largest total the oracle reaches on the pool is 21595 (TCH9 2k4, 'sat' blocks).
  * Ties go to the predecessor that carries the decision bit: 'all 0', 'tern' (generic cost) and 'mag64' (the accelerated
    decoder's |in| cost) tie at nearly every state of every step.  (The two candidates of a step always differ in that
    bit of the low half, so the words themselves are never equal: `<` and `<=` in the select are the same function.  With
    the select turned so that equal metrics go to the other candidate, 58 of this file's 86 tests fail.)
  * Seams: windows of 16 steps (k_xch), 12 (TCH3), 4 + 16 n (K=5 family; the last one 12 or 16 steps in k_nt9, 15 in
    k_rach), a renormalisation after every fourth, the survivor's walk across windows and around the tail-biting wrap, the
    RACH's change of puncturing at step 135, the flush: the single flips visit every position, so every seam.
  * Rows: k_nt9 / k_rach / k_facch3 decode four blocks a wave.  Batches of 1, 3, 5 and 9 with the last batch wrapping run
    waves with 1, 2 and 3 live rows and take every pattern through several rows.
"""
import numpy as np
import pytest

import decoder_patterns as dp

pytestmark = pytest.mark.gpu

FOUR_A_WAVE = (1, 3, 5, 9)
ONE_A_WAVE = (1, 2, 5)
CASES = ([("xch", b) for b in ONE_A_WAVE] + [("rach", b) for b in FOUR_A_WAVE] + [("facch3", b) for b in FOUR_A_WAVE]
         + [(k, b) for k in ("tch3_m0", "tch3_m1") for b in ONE_A_WAVE] + [("facch9", b) for b in FOUR_A_WAVE]
         + [(k, b) for k in ("tch9_0", "tch9_1", "tch9_2") for b in FOUR_A_WAVE])


def _same(names, got, ref_rows, what):
    """every output of every block of a batch equals the oracle's; `what(j)` names block j in the failure message"""
    for name, g, r in zip(names, got, ref_rows):
        g, r = dp.verdict(name, g), dp.verdict(name, r)
        if np.array_equal(g, r):
            continue
        for j in range(r.shape[0]):
            assert np.array_equal(g[j], r[j]), f"{what(j)}: {name} {g[j].tolist()} != {r[j].tolist()}"
        raise AssertionError(f"{what(0)}: {name} shapes {g.shape} / {r.shape}")


@pytest.mark.parametrize("key,batch", CASES, ids=[f"{k}-{b}" for k, b in CASES])
def test_patterns_match_oracle(gpu_api, orc, pkg, decoder, key, batch):
    pats = dp.patterns(pkg, orc, key)
    ref = dp.reference(pkg, orc, key)
    names = dp.SPECS[key].outputs
    n_blocks = 0
    # one entry point call takes a cipher stream for every block or for none: the two halves of the pool walk apart
    for ciphered in (False, True):
        sel = np.array([i for i, p in enumerate(pats) if (p.ciph is not None) == ciphered], int)
        if not sel.size:
            continue
        soft = np.stack([pats[i].soft for i in sel])
        ciph = np.stack([pats[i].ciph for i in sel]) if ciphered else None
        mask = np.array([pats[i].sb_mask for i in sel], np.uint8) if key == "rach" else None
        P = sel.size
        for i0 in range(0, P, batch):
            idx = np.arange(i0, i0 + batch) % P             # the last batch wraps: always `batch` blocks
            got = dp.gpu_decode(gpu_api, key, soft[idx], None if ciph is None else ciph[idx],
                                None if mask is None else mask[idx])
            _same(names, got, [r[sel[idx]] for r in ref],
                  lambda j: f"{decoder} {key} '{pats[sel[idx[j]]].tag}' as block {j} of {batch}")
            n_blocks += batch
    assert n_blocks >= len(pats)


def _tch9_case(orc, mode, seq, n_chan, kind, rng):
    nb = orc.TCH9_BYTES[mode]
    ciph = rng.integers(0, 2, (n_chan * seq, 658), dtype=np.uint8)
    if kind == "sat":
        return rng.choice(np.array([127, -127, -128], np.int8), (n_chan * seq, 662)), ciph, None
    l2 = rng.integers(0, 256, (n_chan, seq, nb), dtype=np.uint8)
    hard = np.concatenate([orc.tch9_encode_seq(l2[ch], mode, rng.integers(0, 2, (seq, 10)), rng.integers(0, 2, (seq, 4)),
                                               ciph[ch * seq:(ch + 1) * seq]) for ch in range(n_chan)])
    return (127 * (1 - 2 * hard.astype(np.int16))).astype(np.int8), ciph, l2


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("seq", [1, 2, 3])
def test_tch9_short_sequences(gpu_api, orc, decoder, mode, seq):
    """Channels of one, two and three bursts: every burst has de-interleaver sources before the channel's start, which
    read as zeros, and no block ever completes.  Five channels, so that channel starts fall in every row of a wave; clean
    (encoded under the cipher stream) and random-sign inputs, each decoded with the stream and without."""
    n_chan = 5
    rng = np.random.default_rng(8300 + 10 * mode + seq)
    for kind in ("clean", "sat"):
        eb, ciph, _ = _tch9_case(orc, mode, seq, n_chan, kind, rng)
        for c in (ciph, None):
            got = gpu_api.tch9_decode_batch(eb, mode, seq, c)
            for ch in range(n_chan):
                sl = slice(ch * seq, (ch + 1) * seq)
                ref = orc.tch9_decode_seq(eb[sl], mode, None if c is None else c[sl])
                _same(("l2", "sacch", "status", "conv"), [g[sl] for g in got], ref,
                      lambda j: f"{decoder} tch9 mode {mode} {kind} {'ciph' if c is not None else 'plain'} "
                                f"channel {ch} of {n_chan}, burst {j} of {seq}")


def test_facch3_cipher_matches_oracle(gpu_api, orc, pkg, decoder):
    """gmr1_hip_facch3_decode_batch with a cipher stream against the oracle given the same stream: 37 groups (nine full
    waves and one live row), clean (encoded under the stream), noisy, junk over the whole int8 range and the drift-maximal
    form.  l2, status bits, crc and conv; the clean and drift-maximal groups decode to what was sent."""
    rng = np.random.default_rng(8400)
    n = 37
    l2 = rng.integers(0, 256, (n, 10), dtype=np.uint8)
    l2[:, 9] &= 0x0F
    s = rng.integers(0, 2, (n, 32), dtype=np.uint8)
    ciph = rng.integers(0, 2, (n, 384), dtype=np.uint8)
    hard = pkg.synth.facch3_encode(l2, s, ciph).reshape(n, 416)
    assert np.array_equal(hard.reshape(n, 4, 104), orc.facch3_encode(l2, s, ciph))
    clean = (127 * (1 - 2 * hard.astype(np.int16))).astype(np.int8)
    noisy = np.clip(55 * (1 - 2 * hard.astype(np.int16)) + rng.normal(0, 45, hard.shape), -128, 127).astype(np.int8)
    junk = rng.integers(-128, 128, hard.shape).astype(np.int8)
    junk[:, ::7] = -128
    drift = np.stack([dp.drift_maximal("facch3", hard[i], dp.burst_mask(pkg, orc, "facch3", ciph[i])) for i in range(n)])
    for tag, eb in (("clean", clean), ("noisy", noisy), ("junk", junk), ("drift", drift)):
        got = gpu_api.facch3_decode_batch(eb, ciph)
        ref = orc.facch3_decode(eb, ciph)
        for name, g, r in zip(("l2", "status", "crc", "conv"), got, ref):
            for j in range(n):
                assert np.array_equal(g[j], r[j]), f"{decoder} facch3 ciph {tag} group {j} of {n}: {name} {g[j]} != {r[j]}"
        if tag in ("clean", "drift"):
            assert np.array_equal(got[0], l2) and np.array_equal(got[1], s) and not got[2].any(), tag
    # the stream matters: without it the same soft bits do not decode
    assert gpu_api.facch3_decode_batch(clean)[2].all()
