"""Cells and inputs of tests/test_gpu_demod4_grid.py: the four-bursts-per-wave demodulator k_rx4g (rx_kernels.hip) at every
format it takes and every window width at which its shape changes.  Everything here is built without a GPU and is seeded.

A cell is (impl, format, extra): 4 samples per symbol, in_len = len * 4 + extra, extra + 1 lags, in a batch of more than
4096 bursts; impl is what demod_kernel_choice (rx_select.h) gives such a call -- 2 = k_rx4g<16,4>, 3 = k_rx4g<8,4> (the
small variant), 4 = k_rx4g<8,4,true> (two training sequences), 0 = k_rx, one step past each limit of the rule.
test_cells_get_the_kernel_the_table_says holds that column to the rule itself."""
from collections import OrderedDict

import numpy as np

from test_gpu_demod_grid import FORMATS, GUARD, LEN

SPS = 4
KINDS = ("matching", "unrelated")
IMPL_NAME = {0: "k_rx", 2: "k_rx4g<16,4>", 3: "k_rx4g<8,4>", 4: "k_rx4g<8,4,true>"}

_TABLE = [
    # two lags; rx_tch3's own window; cw 16 -> 32 and 32 -> 48; +40 is the last small one (stage 64)
    (3, "nt3_speech", (1, 6, 15, 16, 31, 32, 40)),
    (3, "dc2", (12, 36)),                          # +36 is its last small one (stage 64)
    (2, "nt3_speech", (41, 104)),                  # the first generic one (stage 65) and the last (chunk window 128)
    (2, "dc2", (37, 100)),
    (2, "bcch", (1, 16, 80, 84)),                  # +84 is the last (stage 320)
    (2, "dc6", (1, 40, 63, 64, 88)),               # cw 64 -> 80; +88 is in_len 1024
    (4, "nt3_facch", (1, 6, 15, 16, 32)),          # both sequences, drawn per burst; +32 is the last (stage 64)
    (0, "bcch", (85,)), (0, "dc2", (101,)), (0, "nt3_facch", (33,)),
]
CELLS = [(impl, name, extra) for impl, name, extras in _TABLE for extra in extras]
# what the kernel stages of the sync windows where the rule's limit is that figure
STAGE = {("nt3_speech", 40): 64, ("dc2", 36): 64, ("nt3_speech", 41): 65, ("dc2", 37): 65, ("bcch", 84): 320,
         ("nt3_facch", 32): 64}
# one window of len * 4 samples: one lag, where the reference finds no power
ONE_LAG = [(3, "nt3_speech", 0), (2, "bcch", 0), (4, "nt3_facch", 0)]
# one cell per k_rx4g instantiation, for the strided rows and the absent outputs
STRIDED = [(3, "nt3_speech", 16), (2, "dc6", 64), (4, "nt3_facch", 15)]
# gmr1_hip_tch3_rx_batch: one launch (k_rx4g_tch3) up to +40, two launches beyond
TCH3 = [(3, "nt3_speech", 1), (3, "nt3_speech", 6), (3, "nt3_speech", 16), (3, "nt3_speech", 40), (2, "nt3_speech", 41)]
BIG = (2, "dc6", 88)                               # the one batch of 4100 bursts: a full last wave


def cell_id(cell):
    return "impl%d-%s+%d" % cell


def batch_size(cell):
    """4097, 4098 or 4099 bursts, rotated over the cells: the last wave holds 1, 2 or 3 bursts; one cell has 4100"""
    if cell == BIG:
        return 4100
    if cell in ONE_LAG:
        return 4097
    return 4097 + CELLS.index(cell) % 3


def _seed(cell):
    return 94000 + 1000 * FORMATS.index(cell[1]) + cell[2]


class Ref:
    """The oracle's answers to a batch, one array per output; ref[i] is burst i's as orc.demod gave it"""

    def __init__(self, fmt, n):
        self.rv = np.zeros(n, np.int32)
        self.sync_id = np.zeros(n, np.int32)
        self.toa = np.zeros(n, np.float64)
        self.freq_err = np.zeros(n, np.float64)
        self.ebits = np.zeros((n, fmt.ebits), np.int8)
        self.ssyms = np.zeros((n, fmt.length), np.float32)

    def put(self, i, o):
        self.rv[i], self.sync_id[i], self.toa[i], self.freq_err[i] = o["rv"], o["sync_id"], o["toa"], o["freq_err"]
        self.ebits[i], self.ssyms[i] = o["ebits"], o["ssyms"]

    def __getitem__(self, i):
        return dict(rv=int(self.rv[i]), sync_id=int(self.sync_id[i]), toa=float(self.toa[i]), freq_err=float(self.freq_err[i]),
                    ebits=self.ebits[i], ssyms=self.ssyms[i])


def _silent(rng, n, zero_last):
    """-> {burst: value} of the windows without a burst: an all-zero one at each of the four places of some wave (four
    waves, so that each has three ordinary neighbours), one whole wave, a constant one, and the batch's last burst"""
    waves = rng.choice(n // 4, 6, replace=False)
    out = {4 * int(waves[q]) + q: 0.0 for q in range(4)}
    out.update({4 * int(waves[4]) + q: 0.0 for q in range(4)})
    out[4 * int(waves[5]) + int(rng.integers(0, 4))] = 3.0 + 1.0j
    if zero_last:
        out[n - 1] = 0.0
    return out


_cells = OrderedDict()
_KEEP_BYTES = 400 << 20


def cell_inputs(pkg, orc, cell):
    """The cell's windows in their flat array, its two shift arrays and the oracle's answers to both, computed once per
    cell and left alone (the sample arrays of the least recently used cells are dropped beyond 400 MB)"""
    if cell in _cells:
        _cells.move_to_end(cell)
        return _cells[cell]
    impl, name, extra = cell
    n = batch_size(cell)
    fmt = pkg.api.burst_format(name)
    assert fmt.length == LEN[name]
    in_len = fmt.length * SPS + extra
    rng = np.random.default_rng(_seed(cell))
    bits = rng.integers(0, 2, size=(n, fmt.ebits), dtype=np.uint8)
    sid = rng.integers(0, len(fmt.sync), size=n)
    sym = pkg.synth.map_symbols(fmt, bits, sync_id=sid)
    # the burst at `extra` in a window of len * 4 + 2 * extra samples, from which the in_len samples are cut that put it at a lag
    bb = pkg.synth.synth_windows(fmt, sym, SPS, 2 * extra, rng, toa_jitter=0, frac=True, cfo_hz_std=150.0, esn0_db=15.0)
    assert bb.in_len == bb.stride == fmt.length * SPS + 2 * extra
    # a quarter at lags 0 or 1, a quarter at the last two lags, the rest anywhere; drawn per burst, whatever its index
    where = rng.random(n)
    lag = rng.integers(0, extra + 1, n)
    lag = np.where(where < 0.25, rng.integers(0, 2, n), np.where(where < 0.5, extra - rng.integers(0, 2, n), lag))
    lag = np.clip(lag, 0, extra)
    win = np.empty((n, in_len), np.complex64)
    for L in np.unique(lag):
        rows = np.nonzero(lag == L)[0]
        win[rows] = bb.iq[rows, extra - L:extra - L + in_len]
    # a fifth with a constant offset of about the burst's own amplitude: the reference takes the window's mean out
    dc = rng.random(n) < 0.2
    win[dc] += (1.25 * np.exp(2j * np.pi * rng.random(int(dc.sum())))).astype(np.complex64)[:, None]
    silent = _silent(rng, n, zero_last=CELLS.index(cell) % 2 == 0 if cell in CELLS else False)
    for i, v in silent.items():
        win[i] = v
    # one flat array: the windows in a random order of slots, 1 ... 7 samples of 1e6 between them, the first one at sample
    # 0 and the last one up to the array's end
    slot_of = rng.permutation(n)
    gap = rng.integers(1, 8, n)
    gap[0] = 0
    start = np.cumsum(gap) + np.arange(n) * in_len
    iq = np.full(int(start[-1]) + in_len, 1e6, np.complex64)
    offset = start[slot_of].astype(np.uint64)
    for i in range(n):
        iq[int(offset[i]):int(offset[i]) + in_len] = win[i]
    assert offset.min() == 0 and int(offset.max()) + in_len == iq.size
    assert set(np.unique(offset % 4).tolist()) == {0, 1, 2, 3}
    shifts = {"matching": (-bb.cfo * SPS).astype(np.float32), "unrelated": rng.normal(0.0, 0.08, n).astype(np.float32)}
    c = dict(cell=cell, impl=impl, name=name, extra=extra, n=n, sps=SPS, fmt=fmt, dpos=fmt.data_positions(), bits=bits, iq=iq,
             in_len=in_len, offset=offset, lag=lag, dc=dc, silent=silent, shifts=shifts, ref={}, safe={})
    for kind, fs in shifts.items():
        ref = Ref(fmt, n)
        for i in range(n):
            ref.put(i, orc.demod(name, win[i], SPS, float(fs[i])))
        off = np.abs(ref.toa - np.floor(ref.toa + 0.5))           # |toa - round(toa)|, C's roundf on a toa >= 0
        c["ref"][kind], c["safe"][kind] = ref, (ref.rv == 0) & (np.abs(off - 0.5) > GUARD)
    _cells[cell] = c
    kept = 0
    for k in reversed(list(_cells)):
        kept += _cells[k]["iq"].nbytes
        if kept > _KEEP_BYTES and k != cell:
            del _cells[k]
    return c


def check_inputs(c):
    """What the comparisons rest on, on the oracle alone -> dict(safe: the smaller share of safe bursts of the two shifts,
    ber).  At least 85 % of the bursts are safe under either shift; among the safe ones at least 10 were picked at lag 0
    or 1 and at least 10 at the last three lags, in each of the four places of a wave; the oracle gives back the sent bits
    with the matching shift; and the windows without a burst have none for the oracle either."""
    n, extra, fmt = c["n"], c["extra"], c["fmt"]
    tag = cell_id(c["cell"])
    share = []
    for kind in KINDS:
        ref, safe = c["ref"][kind], c["safe"][kind]
        share.append(safe.mean())
        assert safe.mean() >= 0.85, (tag, kind, "only %.3f of the bursts are safe" % safe.mean())
        if extra > 2:
            pick = np.floor(ref.toa + 0.5).astype(int)
            for q in range(4):
                place = safe & (np.arange(n) % 4 == q)
                first, last = int((place & (pick <= 1)).sum()), int((place & (pick >= extra - 2)).sum())
                assert first >= 10 and last >= 10, (tag, kind, "place", q, "picks at the first lags", first, "at the last", last)
        gone = np.array(sorted(c["silent"]))
        assert (ref.rv[gone] == -1).all() and (np.delete(ref.rv, gone) == 0).all(), (tag, kind, np.nonzero(ref.rv)[0])
        for k in ("toa", "freq_err", "ebits", "ssyms"):
            assert not getattr(ref, k)[gone].any(), (tag, kind, k)
    ber = None
    if len(fmt.sync) == 1:
        ref = c["ref"]["matching"]
        ok = ref.rv == 0
        ber = float(((ref.ebits[ok] < 0) != c["bits"][ok].astype(bool)).mean())
        assert ber <= 0.03, (tag, "the oracle gets %.4f of the sent bits wrong" % ber)
    return dict(safe=float(min(share)), ber=ber)
