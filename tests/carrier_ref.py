"""numpy restatement of what the carrier mixer (gmr1_hip_carrier_mix*, include/gmr1_hip.h) computes, independent of
osmo-gmr_amd/csrc/carrier_noise.h: Philox4x32-10 in uint64 arithmetic, the word -> uniform rule, the pair rule in float64;
the carrier phase in extended precision; the mixed carrier in float64 (`mix`) and, for the exact tests, the overlap-add
alone in float32 in list order (`overlap_add_f32`).  Shared by tests/test_carrier_host.py and tests/test_gpu_carrier.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) of integers below 2^32 -> words (..., 4) uint32"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def noise_words(seed, noise_id, n):
    """absolute sample indices n (int64 array) -> (wa, wb) uint32: the two words of each sample"""
    n = np.asarray(n, np.int64)
    j = (n >> 1).astype(np.uint64)                       # arithmetic shift, then the bit pattern
    ctr = np.stack([j & MASK, j >> np.uint64(32), np.full(n.shape, noise_id, np.uint64), np.zeros(n.shape, np.uint64)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    w = philox4x32_10(ctr, np.broadcast_to(key, n.shape + (2,)))
    odd = (n & 1).astype(bool)
    return np.where(odd, w[..., 2], w[..., 0]), np.where(odd, w[..., 3], w[..., 1])


def uniforms(wa, wb):
    """-> (u1 in (0, 1], u2 in [0, 1)) float64, both multiples of 2^-24"""
    return ((wa >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24, (wb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def noise(seed, noise_id, n):
    """-> (z complex128 with unit variance per component, r = |z|)"""
    u1, u2 = uniforms(*noise_words(seed, noise_id, n))
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.exp(2j * np.pi * u2), r


def phase(cfo, n):
    """cfo n reduced to [-pi, pi], in extended precision where numpy has it (x86: 64 mantissa bits) -> float64.
    Also returns |cfo n|, which the bound of the product's rounding in double needs."""
    ld = np.longdouble
    th = ld(cfo) * np.asarray(n, np.int64).astype(ld)
    two_pi = ld(2) * ld("3.14159265358979323846264338327950288")
    return (th - np.rint(th / two_pi) * two_pi).astype(np.float64), np.abs(th).astype(np.float64)


def _clip(pos, ln, first, length):
    """the part of a segment inside [first, first + length): (lo, hi) absolute, hi <= lo if none"""
    return max(pos, first), min(pos + ln, first + length)


def overlap_add_f32(seg_iq, segs, first, length):
    """Step 1 alone, as the kernel does it: float32, one add per component, the segments (src, pos, len) in list order"""
    acc = np.zeros(length, np.complex64)
    for src, pos, ln in segs:
        lo, hi = _clip(int(pos), int(ln), first, length)
        if hi > lo:
            acc[lo - first:hi - first] += seg_iq[src + lo - pos:src + hi - pos]
    return acc


def mix(seg_iq, segs, first, length, sigma=0.0, cfo=0.0, noise_id=0, seed=0):
    """One carrier in float64 -> (x complex128, |acc| before the rotation, r of the noise or None, |cfo n| or None)"""
    acc = np.zeros(length, np.complex128)
    for src, pos, ln in segs:
        lo, hi = _clip(int(pos), int(ln), first, length)
        if hi > lo:
            acc[lo - first:hi - first] += seg_iq[src + lo - pos:src + hi - pos]
    mag = np.abs(acc)
    n = first + np.arange(length, dtype=np.int64)
    turns = None
    if cfo != 0.0:
        ph, turns = phase(cfo, n)
        acc = acc * np.exp(1j * ph)
    r = None
    if sigma != 0.0:
        z, r = noise(seed, noise_id, n)
        acc = acc + sigma * z
    return acc, mag, r, turns
