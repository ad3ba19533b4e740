"""Soft-bit patterns aimed at what the layer-1 Viterbi decoders other than the K=5 BCCH / CCCH one can get wrong -- the
16-bit metric words' headroom, the window seams and the flush, the -128 that negation leaves alone, ties, the rows of a
wave -- and the oracle's answers to them.  TEST INFRASTRUCTURE: numpy, the oracle's and synth's encoders, nothing else.

    patterns(pkg, orc, key)   -> [Pattern(tag, soft, ciph, sb_mask)], built once per decoder
    reference(pkg, orc, key)  -> the oracle's outputs on them, built once per decoder and oracle decoder mode

A decoder is one of KEYS.  `soft` is (nbits,) int8, for TCH9 a five-burst sequence (5, 662); `ciph` the cipher stream
the pattern is decoded with (None: without one); `sb_mask` the RACH's SB mask (None elsewhere).

What a pool holds (tags in quotes):
  constants            'all 0', 'all +127', 'all -127', 'all -128', 'all +1', 'all -1', 'alt +1/-1', 'alt +127/-128'
  saturated codewords  of one random payload: 'cw +-127', 'cw +127/-128' (both in the burst domain) and 'cw drift': after
                       descrambling and deciphering every soft bit is +127 for a coded 0 and -128 for a coded 1, the input
                       that moves a 2*ae - sum(K) metric down fastest (status and SACCH positions: +-127)
  every single flip    'flip<p>': 'cw +-127' with burst position p inverted, every p (TCH9: of burst 2 of the five)
  far from a codeword  64 blocks each of 'sat<i>' (signs over +127 / -127 / -128), 'tern<i>' (-1 / 0 / +1: dense ties in
                       the generic decoder's cost) and 'mag64 <i>' (signs at magnitude 64: dense ties in the accelerated
                       decoder's |in| cost)
  cipher               'cw drift', sat0..15 and 'alt +127/-128' again under a random cipher stream, tagged '... ciph'
  RACH                 everything with the encoder's SB mask; the constants also with mask 0, tagged '... mask 0'
"""
import collections

import numpy as np

KEYS = ("xch", "rach", "facch3", "tch3_m0", "tch3_m1", "facch9", "tch9_0", "tch9_1", "tch9_2")
RACH_MASK = 0xA7
TCH9_SEQ, TCH9_FLIP_BURST = 5, 2
N_FAR, N_FAR_CIPH = 64, 16

Pattern = collections.namedtuple("Pattern", ["tag", "soft", "ciph", "sb_mask"])

# per decoder: bits of a burst, bursts of a pattern, cipher bits of a burst (0: the channel has no cipher), the burst
# positions that carry status / SACCH bits (never scrambled, taken as they come), the names of the decoder's outputs
Spec = collections.namedtuple("Spec", ["nbits", "seq", "nciph", "plain", "outputs"])
_NT9_PLAIN = np.arange(52, 66)                      # status 52..55, SACCH 56..65
SPECS = {
    "xch": Spec(432, 1, 0, np.arange(0), ("l2", "crc", "conv")),
    "rach": Spec(494, 1, 0, np.arange(0), ("rach", "rv", "conv", "crc")),
    "facch3": Spec(416, 1, 384, (np.arange(4)[:, None] * 104 + np.arange(22, 30)[None, :]).ravel(),
                   ("l2", "status", "crc", "conv")),
    "tch3_m0": Spec(212, 1, 208, np.arange(52, 56), ("frame0", "frame1", "status", "conv0", "conv1")),
    "tch3_m1": Spec(212, 1, 208, np.arange(52, 56), ("frame0", "frame1", "status", "conv0", "conv1")),
    "facch9": Spec(662, 1, 658, _NT9_PLAIN, ("l2", "sacch", "status", "crc", "conv")),
    "tch9_0": Spec(662, TCH9_SEQ, 658, _NT9_PLAIN, ("l2", "sacch", "status", "conv")),
    "tch9_1": Spec(662, TCH9_SEQ, 658, _NT9_PLAIN, ("l2", "sacch", "status", "conv")),
    "tch9_2": Spec(662, TCH9_SEQ, 658, _NT9_PLAIN, ("l2", "sacch", "status", "conv")),
}
_SEED = {k: 8100 + i for i, k in enumerate(KEYS)}


def _mode(key):
    return int(key[-1])                             # tch3_m<m>, tch9_<mode>


def payload(key, rng):
    """one random payload, as the encoder's keyword arguments"""
    if key == "xch":
        return dict(l2=rng.integers(0, 256, 24, dtype=np.uint8))
    if key == "rach":
        r = rng.integers(0, 256, 18, dtype=np.uint8)
        r[17] &= 7
        return dict(rach=r)
    if key == "facch3":
        l2 = rng.integers(0, 256, 10, dtype=np.uint8)
        l2[9] &= 0x0F
        return dict(l2=l2, status=rng.integers(0, 2, 32, dtype=np.uint8))
    if key.startswith("tch3"):
        return dict(frame0=rng.integers(0, 256, 10, dtype=np.uint8), frame1=rng.integers(0, 256, 10, dtype=np.uint8),
                    status=rng.integers(0, 2, 4, dtype=np.uint8))
    if key == "facch9":
        l2 = rng.integers(0, 256, 38, dtype=np.uint8)
        l2[37] &= 0x0F
        return dict(l2=l2, sacch=rng.integers(0, 2, 10, dtype=np.uint8), status=rng.integers(0, 2, 4, dtype=np.uint8))
    nb = (18, 30, 60)[_mode(key)]
    return dict(l2=rng.integers(0, 256, (TCH9_SEQ, nb), dtype=np.uint8),
                sacch=rng.integers(0, 2, (TCH9_SEQ, 10), dtype=np.uint8),
                status=rng.integers(0, 2, (TCH9_SEQ, 4), dtype=np.uint8))


def zero_payload(key):
    return {k: np.zeros_like(v) for k, v in payload(key, np.random.default_rng(0)).items()}


def encode(pkg, orc, key, pl, ciph=None, sb_mask=RACH_MASK):
    """payload [, cipher stream] -> hard bits of the burst(s), shaped like a pattern's soft bits"""
    synth = pkg.synth
    c = None if ciph is None else ciph[None]
    if key == "xch":
        return synth.xch_dc12_encode(pl["l2"][None])[0]
    if key == "rach":
        return synth.rach_encode(pl["rach"][None], sb_mask)[0]
    if key == "facch3":
        return synth.facch3_encode(pl["l2"][None], pl["status"][None], c).reshape(416)
    if key.startswith("tch3"):
        return synth.tch3_encode(pl["frame0"][None], pl["frame1"][None], pl["status"][None], _mode(key), c)[0]
    if key == "facch9":
        return orc.facch9_encode(pl["l2"], pl["sacch"], pl["status"], ciph)
    return orc.tch9_encode_seq(pl["l2"], _mode(key), pl["sacch"], pl["status"], ciph)


def burst_mask(pkg, orc, key, ciph=None):
    """The bit every burst position is xored with between the coder and the air: the scrambler's (synth.scramble_mask, laid
    out as the channel lays it out) xor the cipher's.  All these codes are linear and their CRCs start from zero, so it is
    the encoding of the all-zero payload (RACH: with SB mask 0).  0 at the status positions."""
    return encode(pkg, orc, key, zero_payload(key), ciph, sb_mask=0)


def _pm127(hard):
    return (127 * (1 - 2 * hard.astype(np.int16))).astype(np.int8)


def drift_maximal(key, hard, mask):
    """hard bits sent, burst_mask -> burst-domain soft bits that descramble / decipher to +127 (coded 0) / -128 (coded 1)"""
    out = np.where(hard ^ mask, -128, _pm127(hard).astype(np.int16)).astype(np.int8)
    plain = SPECS[key].plain
    out[..., plain] = _pm127(hard[..., plain])
    return out


_patterns = {}
_sent = {}


def sent(pkg, orc, key):
    """the payload of the pool's codewords and flips"""
    patterns(pkg, orc, key)
    return _sent[key]


def patterns(pkg, orc, key):
    if key in _patterns:
        return _patterns[key]
    sp = SPECS[key]
    rng = np.random.default_rng(_SEED[key])
    shape = (sp.nbits,) if sp.seq == 1 else (sp.seq, sp.nbits)
    mask = RACH_MASK if key == "rach" else None
    alt1 = np.broadcast_to(np.where(np.arange(sp.nbits) & 1, -1, 1).astype(np.int8), shape).copy()
    altsat = np.broadcast_to(np.where(np.arange(sp.nbits) & 1, -128, 127).astype(np.int8), shape).copy()
    consts = [(f"all {v:+d}" if v else "all 0", np.full(shape, v, np.int8)) for v in (0, 127, -127, -128, 1, -1)]
    consts += [("alt +1/-1", alt1), ("alt +127/-128", altsat)]
    out = [Pattern(t, s, None, mask) for t, s in consts]
    if key == "rach":
        out += [Pattern(t + " mask 0", s, None, 0) for t, s in consts]

    pl = payload(key, rng)
    _sent[key] = pl
    hard = encode(pkg, orc, key, pl)
    cw = _pm127(hard)
    out.append(Pattern("cw +-127", cw, None, mask))
    out.append(Pattern("cw +127/-128", np.where(hard, -128, 127).astype(np.int8), None, mask))
    out.append(Pattern("cw drift", drift_maximal(key, hard, burst_mask(pkg, orc, key)), None, mask))

    for p in range(sp.nbits):
        f = cw.copy()
        if sp.seq == 1:
            f[p] = -f[p]
        else:
            f[TCH9_FLIP_BURST, p] = -f[TCH9_FLIP_BURST, p]
        out.append(Pattern(f"flip{p}", f, None, mask))

    sat = rng.choice(np.array([127, -127, -128], np.int8), (N_FAR,) + shape)
    tern = rng.integers(-1, 2, (N_FAR,) + shape).astype(np.int8)
    mag64 = (64 * (1 - 2 * rng.integers(0, 2, (N_FAR,) + shape))).astype(np.int8)
    for name, blk in (("sat", sat), ("tern", tern), ("mag64 ", mag64)):
        out += [Pattern(f"{name}{i}", blk[i], None, mask) for i in range(N_FAR)]

    if sp.nciph:
        ciph = rng.integers(0, 2, (2 + N_FAR_CIPH,) + shape[:-1] + (sp.nciph,), dtype=np.uint8)
        hard_c = encode(pkg, orc, key, pl, ciph[0])
        out.append(Pattern("cw drift ciph", drift_maximal(key, hard_c, burst_mask(pkg, orc, key, ciph[0])), ciph[0], None))
        out.append(Pattern("alt +127/-128 ciph", altsat, ciph[1], None))
        out += [Pattern(f"sat{i} ciph", sat[i], ciph[2 + i], None) for i in range(N_FAR_CIPH)]
    for p in out:
        p.soft.setflags(write=False)
    _patterns[key] = out
    return out


def oracle_decode(orc, key, soft, ciph=None, sb_mask=None):
    """one pattern through the oracle -> its outputs in SPECS[key].outputs order (TCH9: one row per burst)"""
    if key == "xch":
        return orc.xch_dc12_decode(soft)
    if key == "rach":
        r, rv, conv, crc = orc.rach_decode(soft, sb_mask)
        return r, rv, conv, np.array(crc, np.int32)
    if key == "facch3":
        return tuple(a[0] for a in orc.facch3_decode(soft[None], None if ciph is None else ciph[None]))
    if key.startswith("tch3"):
        return tuple(a[0] for a in orc.tch3_decode(soft[None], _mode(key), ciph))
    if key == "facch9":
        return orc.facch9_decode(soft, ciph)
    return orc.tch9_decode_seq(soft, _mode(key), ciph)


_reference = {}


def reference(pkg, orc, key):
    """the oracle's outputs on the pool, each stacked over the patterns; once per decoder and oracle decoder mode"""
    k = (key, orc.lib().orc_conv_get_mode())
    if k not in _reference:
        rows = [oracle_decode(orc, key, p.soft, p.ciph, p.sb_mask) for p in patterns(pkg, orc, key)]
        ref = tuple(np.stack([np.asarray(r[i]) for r in rows]) for i in range(len(SPECS[key].outputs)))
        for a in ref:
            a.setflags(write=False)
        _reference[k] = ref
    return _reference[k]


def gpu_decode(api, key, soft, ciph=None, sb_mask=None):
    """a batch of patterns through the product's batch entry point -> outputs like reference()'s rows"""
    sp = SPECS[key]
    n = soft.shape[0]
    if key == "xch":
        return api.xch_dc12_decode_batch(soft)
    if key == "rach":
        return api.rach_decode_batch(soft, sb_mask)
    if key == "facch3":
        return api.facch3_decode_batch(soft, ciph)
    if key.startswith("tch3"):
        return api.tch3_decode_batch(soft, _mode(key), ciph)
    if key == "facch9":
        return api.facch9_decode_batch(soft, ciph)
    got = api.tch9_decode_batch(soft.reshape(n * sp.seq, sp.nbits), _mode(key), sp.seq,
                                None if ciph is None else ciph.reshape(n * sp.seq, sp.nciph))
    return tuple(a.reshape((n, sp.seq) + a.shape[1:]) for a in got)


def verdict(name, a):
    """a CRC output compares as a verdict (passed or not), everything else as it is"""
    return (np.asarray(a) != 0) if name == "crc" else np.asarray(a)
