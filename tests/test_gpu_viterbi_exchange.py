"""The K=5 Viterbi decoder's butterfly exchanges candidates between partner lanes (conv_k5_12.h: each lane adds its
tie-break bit to both candidates it sends on, the min takes the partner's through DPP).  What that could get wrong is
integer and exact: the direction of a tie, the decision bit of the candidate that came from the partner, the window seams
(steps 19 / 20 ... 195 / 196, where the decision half is cleared) and the four flush steps.  Soft-bit patterns aimed at
each, through the layer-1-only calls (soft bits from memory: k_l1 / k_l1_acc) in batches of 5 and of 9 blocks -- one full
wave of four plus a partial one, every block visiting several rows of a wave -- and through the fused call (k_rx4) on five
clean synthetic bursts with both chains in one wave.  l2, crc and conv must equal the oracle's on every block: the oracle's
decoder on the same soft bits (for the fused call, the soft bits it returns), and the whole oracle chain's wherever its
soft bits are the same.

A layer-1-only call decodes one chain, so BCCH and CCCH share a wave in the fused part only; and the fused call makes its
own soft bits (the demodulator's, |v| <= 127), so there the patterns are patterns of the hard bits sent: zeros, -128 and
+-1 reach the decoder through the layer-1-only calls alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLIP_STEPS = (3, 4, 19, 20, 195, 196, 207, 208, 209, 210, 211)
CHAINS = (("bcch", 424, 0), ("ccch", 432, 4))


def _ebit_of_step(k, off):
    """e-bit position of the first coded bit of trellis step k (intra-burst interleaver with N = 53; CCCH: 4 pad bits)"""
    kc = 2 * k
    return 53 * ((5 * kc) & 7) + (kc >> 3) + off


def _hard_patterns(pkg, name, neb, off, seed):
    """[(tag, (neb,) hard bits)]: constants, codewords with one bit flipped at the seams / in the flush, 64 random blocks"""
    rng = np.random.default_rng(seed)
    enc = pkg.synth.bcch_encode if name == "bcch" else pkg.synth.ccch_encode
    out = [("zeros", np.zeros(neb, np.uint8)), ("ones", np.ones(neb, np.uint8)),
           ("alternating", (np.arange(neb) & 1).astype(np.uint8))]
    l2 = rng.integers(0, 256, (len(FLIP_STEPS), 24), dtype=np.uint8)
    cw = enc(l2)
    for i, k in enumerate(FLIP_STEPS):
        b = cw[i].copy()
        b[_ebit_of_step(k, off)] ^= 1
        out.append((f"flip{k}", b))
    rnd = rng.integers(0, 2, (64, neb), dtype=np.uint8)
    out += [(f"random{i}", rnd[i]) for i in range(64)]
    return out


def _soft_patterns(pkg, name, neb, off, seed):
    """[(tag, (neb,) int8 soft bits)] for the layer-1-only calls"""
    rng = np.random.default_rng(seed + 1000)
    hard = dict(_hard_patterns(pkg, name, neb, off, seed))
    alt = np.where(np.arange(neb) & 1, -1, 1).astype(np.int8)
    cw = (127 * (1 - 2 * hard["flip3"].astype(np.int16))).astype(np.int8)
    erased = cw.copy()
    erased[1::2] = 0
    out = [("all zero", np.zeros(neb, np.int8)), ("all +127", np.full(neb, 127, np.int8)),
           ("all -127", np.full(neb, -127, np.int8)), ("all -128", np.full(neb, -128, np.int8)),
           ("alternating +-1", alt), ("every second erased", erased)]
    for k in FLIP_STEPS:
        out.append((f"flip{k}", (127 * (1 - 2 * hard[f"flip{k}"].astype(np.int16))).astype(np.int8)))
    rnd = rng.integers(-128, 128, (64, neb)).astype(np.int8)
    out += [(f"random{i}", rnd[i]) for i in range(64)]
    return out


_pool = {}


def _l1_pool(pkg, orc, mode):
    """per chain: (tags, soft bits (P, neb), the oracle's (l2, crc, conv)) -- computed once per decoder mode"""
    if mode not in _pool:
        pool = {}
        for ci, (name, neb, off) in enumerate(CHAINS):
            pats = _soft_patterns(pkg, name, neb, off, 7100 + ci)
            eb = np.stack([p for _, p in pats])
            ref = (orc.bcch_decode if name == "bcch" else orc.ccch_decode)(eb)
            for a in ref:
                a.setflags(write=False)
            pool[name] = ([t for t, _ in pats], eb, ref)
        _pool[mode] = pool
    return _pool[mode]


@pytest.mark.parametrize("batch", [5, 9])
def test_l1_patterns_match_oracle(gpu_api, orc, pkg, decoder, batch):
    pool = _l1_pool(pkg, orc, decoder)
    for name, neb, off in CHAINS:
        tags, eb, ref = pool[name]
        dec = gpu_api.bcch_decode_batch if name == "bcch" else gpu_api.ccch_decode_batch
        P = eb.shape[0]
        if name == "bcch":
            # the patterns are what they claim: a codeword with one flipped bit still passes its CRC
            assert not ref[1][tags.index("flip3"):tags.index("flip211") + 1].any()
        for i0 in range(0, P, batch):
            idx = np.arange(i0, i0 + batch) % P              # the last batch wraps: always `batch` blocks
            l2, crc, conv = dec(eb[idx])
            for j, i in enumerate(idx):
                what = f"{decoder} {name} '{tags[i]}' as block {j} of {batch}"
                assert np.array_equal(l2[j], ref[0][i]), what + ": l2"
                assert crc[j] == ref[1][i], what + ": crc"
                assert conv[j] == ref[2][i], what + ": conv"


def _fused_batch(pkg, hard_by_kind, kinds, rng):
    """five clean bursts (integer timing, no noise, no offset) carrying the given hard bits -> (iq, offset, kind)"""
    sps = 4
    fmt = [pkg.api.burst_format("bcch"), pkg.api.burst_format("dc6")]
    win = [20 * sps, 10 * sps]
    stride = [-(-(234 * sps + w) // 16) * 16 for w in win]
    sizes = np.array([stride[k] for k in kinds], np.uint64)
    offset = np.zeros(len(kinds), np.uint64)
    offset[1:] = np.cumsum(sizes)[:-1]
    iq = np.zeros(int(sizes.sum()), np.complex64)
    for k in (0, 1):
        rows = np.nonzero(kinds == k)[0]
        sym = pkg.synth.map_symbols(fmt[k], hard_by_kind[k][:rows.size])
        bb = pkg.synth.synth_windows(fmt[k], sym, sps, win[k], rng, esn0_db=np.full(rows.size, 200.0), stride=stride[k])
        idx = offset[rows][:, None].astype(np.int64) + np.arange(stride[k])[None, :]
        iq[idx] = bb.iq
    return iq, offset


def test_fused_patterns_match_oracle(gpu_api, orc, pkg, decoder):
    kinds = np.array([0, 1, 1, 0, 1], np.uint8)              # both chains in the full wave, one burst in a partial wave
    rng = np.random.default_rng(7300)
    pats = [_hard_patterns(pkg, name, neb, off, 7200 + ci) for ci, (name, neb, off) in enumerate(CHAINS)]
    tags = [t for t, _ in pats[0]]
    fixed = [t for t in tags if not t.startswith("random")]
    rnd = [t for t in tags if t.startswith("random")]
    by = [dict(p) for p in pats]
    # one batch per fixed pattern (all five bursts carry it), then the random blocks five at a time
    batches = [(t, [np.stack([by[k][t]] * 5) for k in (0, 1)]) for t in fixed]
    for i0 in range(0, len(rnd), 5):
        ts = [rnd[(i0 + j) % len(rnd)] for j in range(5)]
        batches.append((ts[0] + "..", [np.stack([by[k][t] for t in ts]) for k in (0, 1)]))
    n_same = n_bursts = 0
    for tag, hard in batches:
        iq, offset = _fused_batch(pkg, hard, kinds, rng)
        got = gpu_api.rx_bcch_ccch_batch(iq, offset, kinds, sps=4)
        ref = orc.demod_decode_batch(iq, offset, kinds, sps=4)
        what = f"{decoder} '{tag}'"
        assert np.array_equal(got["rv"], ref["rv"]) and not got["rv"].any(), what + ": rv"
        # The decoder is held to the oracle's decoder on the SAME soft bits, on every burst: the ones the fused call itself
        # returned.  (Its demodulator may round a soft bit one step away from the oracle's float stage -- the parity contract
        # of tests/test_gpu_rx.py; one soft bit of 126 read as 127 moves the generic decoder's path metric on 'alternating'
        # from the whole oracle chain's 6659 to 6660 with the payload unchanged.)
        for i, k in enumerate(kinds):
            neb = CHAINS[k][1]
            l2, crc, conv = (orc.bcch_decode if k == 0 else orc.ccch_decode)(got["ebits"][i:i + 1, :neb])
            assert np.array_equal(got["l2"][i], l2[0]), f"{what} burst {i}: l2"
            assert got["crc"][i] == crc[0], f"{what} burst {i}: crc"
            assert got["conv"][i] == conv[0], f"{what} burst {i}: conv"
        # and to the whole oracle chain wherever the two float stages agree on every soft bit; elsewhere by a step at most
        d = np.abs(got["ebits"].astype(int) - ref["ebits"].astype(int))
        assert d.max() <= 1, what + f": soft bits differ by {d.max()}"
        same = ~d.any(axis=1)
        n_same += int(same.sum())
        n_bursts += same.size
        for key in ("l2", "crc", "conv"):
            assert np.array_equal(got[key][same], ref[key][same]), what + ": " + key
        if tag.startswith("flip"):
            assert not got["crc"].any(), what + ": a single flipped bit must be corrected"
    print(f"fused patterns ({decoder}): all soft bits identical to the oracle's on {n_same} of {n_bursts} bursts")
    # the whole-chain check is not idle: 85 % of noisy bursts have all soft bits identical (DESIGN.md section 6,
    # tests/test_gpu_rx.py); clean ones no fewer, less three standard deviations of this sample
    assert n_same / n_bursts > 0.85 - 3.0 * np.sqrt(0.85 * 0.15 / n_bursts)
