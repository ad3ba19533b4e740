"""The pool of tests/decoder_patterns.py is what it claims to be -- conditions on the test inputs, checked on the oracle alone
(no GPU), in both of its decoder modes: the saturated codewords are codewords, every single flip is one the code corrects,
the -128 quirk is there, and the far-from-codeword blocks drive the path metric as high as the headroom arguments of
tests/test_gpu_decoder_patterns.py need them to."""
import numpy as np
import pytest

import decoder_patterns as dp

MODES = ((0, "generic"), (1, "acc"))

# the oracle's largest generic-mode path metric over 64 blocks of random signs of +127 / -127 / -128, as measured when the
# pool was written; the pool must keep reaching at least half of each
FAR_CONV = {"tch9_0": 20615, "facch3": 12284, "facch9": 11748, "rach": 7623}


def _by_tag(pkg, orc, key):
    pats = dp.patterns(pkg, orc, key)
    ref = dp.reference(pkg, orc, key)
    names = dp.SPECS[key].outputs
    idx = {p.tag: i for i, p in enumerate(pats)}
    assert len(idx) == len(pats), "tags are unique"
    return pats, idx, {n: ref[j] for j, n in enumerate(names)}


def _payload_back(key, out, i, sent, class1_only=False):
    """the decoded payload of pattern i is what was sent (and its CRCs pass, where the channel has any)"""
    if key.startswith("tch9"):
        # a block leaves the inter-burst de-interleaver two bursts after its first burst
        return np.array_equal(out["l2"][i][2:], sent["l2"][:-2])
    if key.startswith("tch3"):
        # bytes 0..5 of a frame are its 48 coded class-1 bits; the 32 class-2 bits behind them are sent uncoded
        nb = 6 if class1_only else 10
        return (np.array_equal(out["frame0"][i][:nb], sent["frame0"][:nb])
                and np.array_equal(out["frame1"][i][:nb], sent["frame1"][:nb]))
    if key == "rach":
        return np.array_equal(out["rach"][i], sent["rach"]) and out["rv"][i] == 0 and not out["crc"][i].any()
    return np.array_equal(out["l2"][i], sent["l2"]) and out["crc"][i] == 0


def _convs(key, out, i):
    names = ("conv0", "conv1") if key.startswith("tch3") else ("conv",)
    return np.concatenate([np.atleast_1d(out[n][i]) for n in names])


@pytest.mark.parametrize("key", dp.KEYS)
def test_pool_is_what_it_claims(pkg, orc, key):
    sp = dp.SPECS[key]
    for mode, mname in MODES:
        with orc.conv_mode(mode):
            pats, idx, out = _by_tag(pkg, orc, key)
            sent = dp.sent(pkg, orc, key)
            what = f"{mname} {key}"
            for p in pats:
                assert p.soft.dtype == np.int8 and p.soft.shape[-1] == sp.nbits
                assert (p.ciph is None) or p.ciph.shape[-1] == sp.nciph
            assert sum(p.tag.startswith("flip") for p in pats) == sp.nbits
            # the saturated codewords come back as sent; in generic mode (cost: |in| of every disagreeing soft bit) at no cost
            for tag in ("cw +-127", "cw drift") + (("cw drift ciph",) if sp.nciph else ()):
                assert _payload_back(key, out, idx[tag], sent), f"{what} '{tag}': payload"
                if mode == 0:
                    full = _convs(key, out, idx[tag])[-3:] if sp.seq > 1 else _convs(key, out, idx[tag])
                    assert not full.any(), f"{what} '{tag}': conv {full}"
            # the drift-maximal codeword is +127 / -128 behind the scrambler: -128 wherever the coded bit is 1
            hard = dp.encode(pkg, orc, key, sent)
            drift = pats[idx["cw drift"]].soft
            coded1 = (hard ^ dp.burst_mask(pkg, orc, key)).astype(bool)
            coded1[..., sp.plain] = False
            assert (drift[coded1] == -128).all() and (np.abs(drift[~coded1].astype(int)) == 127).all()
            assert np.array_equal(drift[~coded1] < 0, hard[~coded1].astype(bool))
            # every single flip
            flips = [idx[f"flip{p}"] for p in range(sp.nbits)]
            lost = [p for p, i in enumerate(flips) if not _payload_back(key, out, i, sent, class1_only=True)]
            print(f"{what}: {len(lost)} of {sp.nbits} single flips not corrected"
                  + (" (class-1 bytes)" if key.startswith("tch3") else ""))
            if not key.startswith("tch3"):
                # TCH3 has no CRC, its class-2 bits are uncoded and the oracle's tail-biting decoder itself does not
                # correct every flip of the class-1 part: nothing to assert there
                assert not lost, f"{what}: flips {lost}"
            cmax = max(int(_convs(key, out, i).max()) for i in range(len(pats)))
            far = max(int(_convs(key, out, idx[f"sat{i}"]).max()) for i in range(dp.N_FAR))
            print(f"{what}: {len(pats)} patterns, {len(pats) * sp.seq} bursts, largest conv {cmax} (random signs: {far})")
            if mode == 0 and key in FAR_CONV:
                assert far >= FAR_CONV[key] // 2, f"{what}: random signs reach conv {far} only"
            if key == "xch":
                # (int8)(-v) leaves -128 alone: a codeword sent as +127 / -128 does not decode at cost 0
                i = idx["cw +127/-128"]
                assert out["conv"][i] > 0, f"{what}: conv {out['conv'][i]}"
                print(f"{what}: 'cw +127/-128' conv {out['conv'][i]}")


def test_burst_mask_is_the_scrambler(pkg, orc):
    """what drift_maximal takes for the scrambler is synth.scramble_mask, where the channel's layout is plain to write down"""
    scr = pkg.synth.scramble_mask
    assert np.array_equal(dp.burst_mask(pkg, orc, "xch"), scr(432))
    for key in ("tch3_m0", "tch3_m1"):
        assert np.array_equal(np.delete(dp.burst_mask(pkg, orc, key), np.arange(52, 56)), scr(208))
    f3 = dp.burst_mask(pkg, orc, "facch3").reshape(4, 104)
    assert all(np.array_equal(np.delete(f3[b], np.arange(22, 30)), scr(96)) for b in range(4))
    for key in ("facch9", "tch9_0", "tch9_1", "tch9_2"):
        m = dp.burst_mask(pkg, orc, key).reshape(-1, 662)
        assert all(np.array_equal(np.delete(row, dp.SPECS[key].plain), scr(648)) for row in m)
    # and with a cipher stream: xor, at the cipher's own positions (NT9: the SACCH bits are ciphered, the status bits not)
    rng = np.random.default_rng(5)
    c = rng.integers(0, 2, 658, dtype=np.uint8)
    m = dp.burst_mask(pkg, orc, "facch9", c)
    assert np.array_equal(np.delete(m, np.arange(52, 56)), np.delete(dp.burst_mask(pkg, orc, "facch9"), np.arange(52, 56)) ^ c)
