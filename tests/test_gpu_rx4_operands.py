"""The fused batch kernel asks for pass 2's and the decoder's per-lane operands in one batch, by each burst's kind, before
it knows which of a wave's bursts were found or whose speculated pick held (k_rx4's OPS_AHEAD): waves of
every BCCH / CCCH kind pattern, ragged last waves, a burst that is not found at each place among found ones, and bursts
whose pick is not the speculated one beside bursts whose pick is -- against the CPU oracle, never against the library
itself, at the headline geometry (windows of 1016 / 976 samples, 4 samples per symbol), in both decoder modes.

The batch entry gives a wave FOUR bursts only above 4096 bursts (one burst per wave below: launch_rx_t), so the batches are
index lists into a pool of 58 windows (offsets may repeat): the oracle runs on the pool once per decoder, the special waves
stand at the head of the list, a filler brings it past 4096, and n = 4096 + {1, 2, 3, 5, 7} leaves every ragged last wave.
n = 1, 2, 3, 5, 7 themselves run as well (one burst per wave: the hoisted requests of the three shadow bursts).

Which bursts are mis-speculated is worked out on the CPU: the kernel speculates the pick as the lag of the largest sync
correlation magnitude, so the bursts wanted are those whose oracle round(toa) is another lag (seeds recorded below, the
condition re-checked in the fixture with the correlation restated in numpy)."""
import numpy as np
import pytest

import workloads

pytestmark = pytest.mark.gpu

SPS = 4
SEEDS = (71, 75)                 # workloads.bcch_ccch_mix(n=28): 4 BCCH + 24 CCCH bursts each, Es/N0 6 / 10 / 20 dB
# (seed, burst): the oracle's round(toa) is NOT the lag of the largest correlation magnitude, by a margin of 4 % or more
# between the two largest magnitudes (three CCCH bursts, one BCCH burst; chosen with the oracle on the CPU)
MISSED = ((71, 18), (71, 22), (71, 27), (75, 14))
# sync chunks (first symbol, training symbols) of the BCCH burst and of the CCCH's DC6 burst (nb.c:36-41, 94-99)
SYNC = {0: ((28, (0, 2, 2, 0, 0, 0, 2, 0, 2, 2, 2)), (119, (2, 2, 0)), (197, (2, 2, 0))),
        1: ((28, (0, 0, 0, 2, 2, 0, 2)), (119, (0, 3, 0)), (197, (3, 1, 1)))}
FIELDS = ("rv", "l2", "crc", "conv", "toa", "freq_err", "ebits", "ssyms")


def _corr_mag(x, kind):
    """sum over the sync chunks of |sum_n conj(ref_n) e^{-j pi/4 n} x[(pos + n) sps + lag]| on the window less its mean
    (pi4cxpsk.c:125-237), per lag, in float64"""
    x = x.astype(np.complex128)
    x = x - x.mean()
    w = x.size - 234 * SPS + 1
    out = np.zeros(w)
    lags = np.arange(w)
    for pos, syms in SYNC[kind]:
        n = np.arange(len(syms))
        c = np.conj(np.exp(0.5j * np.pi * np.asarray(syms))) * np.exp(-0.25j * np.pi * n)
        out += np.abs((c[None, :] * x[(pos + n)[None, :] * SPS + lags[:, None]]).sum(axis=1))
    return out


@pytest.fixture(scope="module")
def pool(pkg, orc):
    """58 windows: two seeded mixes, an all-zero window (BCCH kind) and a constant one (CCCH kind), which the reference
    finds no sync in (test_gpu_rx.py::test_fused_rx_degenerate_inputs builds them so)"""
    iqs, offs, kinds, l2s, tag = [], [], [], [], []
    base = 0
    for seed in SEEDS:
        wl = workloads.bcch_ccch_mix(pkg, n=28, seed=seed)
        iqs.append(wl["iq"])
        offs.append(wl["offset"] + np.uint64(base))
        kinds.append(wl["kind"])
        l2s.append(wl["l2"])
        tag += [(seed, i) for i in range(28)]
        base += wl["iq"].size
    iqs.append(np.zeros(1024, np.complex64))
    iqs.append(np.full(1024, 3.0 + 1.0j, np.complex64))
    offs.append(np.array([base, base + 1024], np.uint64))
    kinds.append(np.array([0, 1], np.uint8))
    tag += [("zeros", 0), ("const", 0)]
    P = dict(iq=np.concatenate(iqs), offset=np.concatenate(offs), kind=np.concatenate(kinds), l2=np.concatenate(l2s), tag=tag)
    n = P["kind"].size
    assert n == 58
    # the oracle, once per decoder (the payload bytes differ only where the two decoders do)
    P["ref"] = {}
    for name, mode in (("generic", 0), ("acc", 1)):
        with orc.conv_mode(mode):
            P["ref"][name] = orc.demod_decode_batch(P["iq"], P["offset"], P["kind"], sps=SPS)
    ref = P["ref"]["acc"]
    assert list(ref["rv"][56:]) == [-1, -1] and not ref["rv"][:56].any()
    # speculated pick (largest magnitude) against the oracle's pick
    d = np.round(ref["toa"]).astype(int)
    p = np.zeros(n, int)
    margin = np.zeros(n)
    for i in range(56):
        k = int(P["kind"][i])
        o = int(P["offset"][i])
        m = _corr_mag(P["iq"][o:o + (1016, 976)[k]], k)
        p[i] = int(np.argmax(m))
        s = np.sort(m)
        margin[i] = s[-1] / s[-2]
    P["missed"] = [tag.index(t) for t in MISSED]
    for i in P["missed"]:
        assert p[i] != d[i] and abs(p[i] - d[i]) == 1 and margin[i] > 1.04, (tag[i], p[i], d[i], margin[i])
    # bursts whose pick IS the speculated one, as clearly
    P["held"] = [i for i in range(56) if p[i] == d[i] and margin[i] > 1.04]
    assert len([i for i in P["held"] if P["kind"][i] == 0]) >= 3 and len([i for i in P["held"] if P["kind"][i] == 1]) >= 8
    assert {int(P["kind"][i]) for i in P["missed"]} == {0, 1}
    return P


def _cycle(xs):
    i = 0
    while True:
        yield xs[i % len(xs)]
        i += 1


def _order(P):
    """pool indices of the long batches: the special waves of four, then a filler over the whole pool"""
    found = list(range(56))
    by_kind = [_cycle([i for i in found if P["kind"][i] == k]) for k in (0, 1)]
    held, missed = _cycle(P["held"]), _cycle(P["missed"])
    anyf = _cycle(found)
    out = []
    for pat in range(16):                              # every BCCH / CCCH pattern of a wave
        out += [next(by_kind[(pat >> q) & 1]) for q in range(4)]
    for nf in (56, 57):                                # a burst that is not found at each place among found ones
        for pos in range(4):
            out += [nf if q == pos else next(anyf) for q in range(4)]
    out += [56, 57, 57, 56]                            # ... and a wave that finds nothing
    for pat in (1, 2, 4, 8, 3, 6, 12, 9, 5, 10, 7, 14, 15):   # bit q: burst q's pick is NOT the speculated one
        out += [next(missed) if (pat >> q) & 1 else next(held) for q in range(4)]
    out += [56, next(missed), next(held), 57]          # both kinds of exception in one wave
    assert len(out) % 4 == 0 and len(out) < 512
    allp = _cycle(list(range(58)))
    while len(out) < 4096 + 8:
        out.append(next(allp))
    return np.asarray(out)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(got, idx, P, decoder, label):
    ref = P["ref"][decoder]
    n = idx.size
    # a burst's outputs do not depend on where in the batch, beside whom, it stands: every copy equals the first
    first = {}
    for j, i in enumerate(idx):
        first.setdefault(int(i), j)
    rep = np.asarray([first[int(i)] for i in idx])
    for f in FIELDS:
        assert np.array_equal(_bits(got[f]), _bits(got[f][rep])), f"{label}: {f} of one window differs between its copies"
    # the first copies against the oracle, at test_gpu_rx.py's tolerances
    u = np.asarray(sorted(first))
    g = {f: got[f][[first[int(i)] for i in u]] for f in FIELDS}
    r = {f: ref[f][u] for f in FIELDS}
    kinds = P["kind"][u]
    assert np.array_equal(g["rv"], r["rv"]), f"{label}: rv differs"
    nf = r["rv"] != 0
    for f in ("l2", "crc", "conv", "toa", "freq_err"):
        assert np.array_equal(g[f][nf], r[f][nf]), f"{label}: {f} of a burst that was not found"
    assert not g["ebits"][nf].any() and not g["ssyms"][nf].any(), f"{label}: soft outputs of a burst that was not found"
    fd = ~nf
    dtoa = np.abs(g["toa"] - r["toa"])
    assert dtoa[fd].max(initial=0.0) < 16.0 / 1024.0, f"{label}: toa differs by {dtoa[fd].max()}"
    flip = fd & (np.round(g["toa"]) != np.round(r["toa"]))
    # (test_gpu_rx.py bounds the flipped picks by 0.5 % of the bursts; of at most 56 that is one)
    assert flip.sum() <= 1, f"{label}: {flip.sum()} sample-pick flips among {fd.sum()} bursts"
    same = fd & ~flip
    dss = np.abs(g["ssyms"][same] - r["ssyms"][same])
    dss = np.minimum(dss, np.abs(dss - 4.0))
    assert dss.max(initial=0.0) < 1e-4, f"{label}: soft symbols differ by {dss.max()}"
    assert np.abs(g["freq_err"][same] - r["freq_err"][same]).max(initial=0.0) < 1e-5, f"{label}: freq_err"
    deb = np.abs(g["ebits"].astype(int) - r["ebits"].astype(int))
    deb[~same] = 0
    if deb.max(initial=0) > 1:
        # a symbol on the midpoint between two constellation points within the soft-symbol tolerance swaps the roles of the
        # nearest point and its neighbour: the weakest soft bit (|value| 63) changes sign and nothing else (test_gpu_rx.py)
        fmts = [P["fmt"][0], P["fmt"][1]]
        pos = [np.concatenate([np.arange(a, a + l) for a, l in f.data]) for f in fmts]
        for b, e in zip(*np.nonzero(deb > 1)):
            sym = pos[kinds[b]][e // 2]
            frac = abs(abs(float(r["ssyms"][b, sym])) % 1.0 - 0.5)
            assert frac < 1e-4, f"{label}: window {P['tag'][u[b]]} bit {e}: {g['ebits'][b, e]} vs {r['ebits'][b, e]}"
            assert abs(abs(int(g["ebits"][b, e])) - 63) <= 1 and abs(abs(int(r["ebits"][b, e])) - 63) <= 1, (label, b, e)
        assert (deb > 1).sum() <= 1, f"{label}: {(deb > 1).sum()} midpoint symbols"
    if same.any():
        assert ((deb[same] != 0) & (deb[same] <= 1)).mean() < 1e-3, f"{label}: {(deb[same] != 0).mean():.2e} of soft bits differ"
    eq = same & np.all(g["ebits"] == r["ebits"], axis=1)
    for f in ("l2", "crc", "conv"):
        assert np.array_equal(g[f][eq], r[f][eq]), f"{label}: {f} differs on identical soft bits"
    ok = fd & ((g["crc"] == 0) | (r["crc"] == 0))
    assert np.array_equal(g["crc"][ok], r["crc"][ok]), f"{label}: CRC verdicts differ"
    assert np.array_equal(g["l2"][ok], r["l2"][ok]), f"{label}: decoded payloads differ"
    sent = u < 56
    good = sent & (g["crc"] == 0) & fd
    assert np.array_equal(g["l2"][good], P["l2"][u[good]]), f"{label}: payload is not what was sent"
    return dict(n=n, windows=int(u.size), flips=int(flip.sum()), soft_bits_identical=int(eq.sum()), crc_ok=int(good.sum()))


def _run(gpu_api, P, idx):
    return gpu_api.rx_bcch_ccch_batch(P["iq"], P["offset"][idx], P["kind"][idx], sps=SPS)


@pytest.fixture(scope="module")
def pool_fmt(pool, pkg):
    pool["fmt"] = [pkg.api.burst_format("bcch"), pkg.api.burst_format("dc6")]
    return pool


@pytest.mark.parametrize("extra", [1, 2, 3, 5, 7])
def test_four_burst_waves_every_pattern_and_exception(gpu_api, pool_fmt, decoder, extra):
    """n = 4096 + extra: four bursts a wave, the special waves at the head, a ragged last wave of extra % 4 bursts"""
    P = pool_fmt
    idx = _order(P)[:4096 + extra]
    st = _check(_run(gpu_api, P, idx), idx, P, decoder, f"n={idx.size} {decoder}")
    print("rx4 operands:", st)
    assert st["windows"] == 58 and st["crc_ok"] >= 45


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
def test_small_batches(gpu_api, pool_fmt, decoder, n):
    """n = 1, 2, 3, 5, 7: one burst a wave (three shadow bursts' requests beside it), both kinds, a burst that is not found
    and mis-speculated picks among them"""
    P = pool_fmt
    ccch_held = [i for i in P["held"] if P["kind"][i] == 1]
    bcch_held = [i for i in P["held"] if P["kind"][i] == 0]
    order = [ccch_held[0], P["missed"][3], 56, P["missed"][0], bcch_held[0], 57, ccch_held[1]]
    assert P["kind"][P["missed"][3]] == 0 and P["kind"][P["missed"][0]] == 1
    idx = np.asarray(order[:n])
    _check(_run(gpu_api, P, idx), idx, P, decoder, f"n={n} {decoder}")
