"""The folded FCCH rough sweep (k_fcch_sweep<NT, true>) at the geometries, edges and fallbacks test_gpu_fcch.py does not reach.

Every case is checked against the CPU oracle (orc_fcch_rough / orc_fcch_rough_multi): toa and rv per stream, peak counts and
ranked lists per window, identical.  A case's streams index a few distinct windows (stream i reads window i % W, so neighbouring
streams differ): a launch is large enough to be folded (more than 512 work-groups) while the oracle and the inputs stay small.
Every rough window is checked first against a float64 restatement of the sweep: its best 5-lag window beats the runner-up by a
clear relative margin and its toa is clear of a rounding boundary, so that no case is decided by last bits (the folded tile, the
tile that gives up and the two-kernel form group the taps of the lags at a tile's edge differently).

The fallbacks run in child processes on the profiling build, every input poisoned (GMR1_HIP_FCCH_POISON=1: a lag that no tile
wrote decides the pick), with the tiles of a folded launch made to give up all of them, some of them or the last one only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.path.join(ROOT, "osmo-gmr_amd", "libgmr1_hip_prof.so")
TILE_STEP = 2044                          # kTileStep (fcch_kernels.hip): lags a tile's windows start at
BURST = {"fcch": (117, 0.32), "fcch3_lband": (468, 0.32), "fcch3_sband": (468, 0.16)}


# ---- float64 restatement of orc_fcch_rough (oracle/orc_sdr.c, orc_3p.c) --------------------------------------------------
def rough_ref(x, sps, fs=0.0, which="fcch"):
    """normalise over the whole window, decimate, shift, correlate with the dual chirp, |.|^2, 5-lag sums.
    Returns (best window start, its relative margin over the runner-up, toa in samples before rounding)."""
    ntaps, freq = BURST[which]
    x = np.asarray(x, np.complex128)
    mu = x.mean()
    sd = np.sqrt(np.mean(np.abs(x - mu) ** 2)) or 1.0
    d = (x[: (x.size // sps) * sps: sps] - mu) / sd
    if fs:
        d = d * np.exp(1j * np.float64(fs) * np.arange(d.size))
    pos = np.arange(ntaps) - ntaps / 2.0
    r = np.sqrt(2.0) * np.cos(freq * 2.0 * np.pi / ntaps * pos * pos)
    e = np.abs(np.correlate(d, r, "valid")) ** 2
    w5 = np.convolve(e, np.ones(5), "valid")
    best = int(np.argmax(w5))
    runner = np.max(np.delete(w5, best)) if w5.size > 1 else 0.0
    k = np.arange(best, best + 5)
    return best, float((w5[best] - runner) / w5[best]), float(np.sum(e[k] * k) / np.sum(e[k])) * sps


def _clear(x, sps, fs=0.0, which="fcch", want=None):
    best, margin, t = rough_ref(x, sps, fs, which)
    return (margin > 1e-3 and abs(t - np.floor(t) - 0.5) > 0.05 and (want is None or best == want)), best, margin


# ---- cases -------------------------------------------------------------------------------------------------------------
def _window(pkg, rng, L, sps, which="fcch", first=None, snr_db=None, cfo=300.0):
    ntaps, freq = BURST[which]
    if first is None:
        first = int(rng.integers(0, L - ntaps * sps))
    x, _ = pkg.synth.synth_fcch_stream(L, sps, rng, snr_db=float(rng.uniform(3.0, 12.0)) if snr_db is None else snr_db,
                                       cfo_hz=float(rng.uniform(-cfo, cfo)), first=first, period_sym=10 ** 7,
                                       freq=freq, length=ntaps)
    return x


def _rough_case(name, wins, n, L, sps, which="fcch", fs=None, odd=False, want=None):
    """n streams over the distinct windows `wins` (stream i reads window i % W), laid out in one buffer at even (or odd)
    offsets; fs: per-window freq_shift; want: per-window intended best window start (None: any)"""
    W = len(wins)
    gap = L + 64 + (L & 1)
    buf = np.zeros(W * gap + 2, np.complex64)
    woff = np.array([w * gap + (1 if odd else 0) for w in range(W)], np.uint64)
    for w, x in enumerate(wins):
        buf[int(woff[w]):int(woff[w]) + L] = x
    return dict(name=name, kind="rough", iq=buf, off=woff[np.arange(n) % W], win=np.arange(n) % W, woff=woff, len=L, sps=sps,
                which=which, fs=None if fs is None else np.asarray(fs, np.float32)[np.arange(n) % W],
                want=None if want is None else [None if v is None else int(v) for v in want])


def _clear_windows(pkg, rng, W, L, sps, which="fcch", fs=None, dc=None):
    """W distinct one-chirp windows, each redrawn until its pick is clear (fs, dc: per window)"""
    out = []
    for w in range(W):
        f = 0.0 if fs is None else float(fs[w])
        while True:
            x = _window(pkg, rng, L, sps, which)
            if dc is not None:
                x = (x + np.complex64(dc[w])).astype(np.complex64)
            if _clear(x, sps, f, which)[0]:
                break
        out.append(x)
    return out


def _edge_windows(pkg, rng, L, sps, targets):
    """one window per intended best window start: a single strong chirp (CFO 0) placed, and its noise redrawn, until the
    restatement's best window starts exactly there by a clear margin"""
    out = []
    for w0 in targets:
        for attempt in range(400):
            first = sps * (w0 + 2) + (attempt % 7 - 3) * max(1, sps // 2)
            x = _window(pkg, rng, L, sps, first=first, snr_db=15.0, cfo=0.0)
            if _clear(x, sps, want=w0)[0]:
                break
        else:
            raise AssertionError("no clear window at %d" % w0)
        out.append(x)
    return out


def build_cases(pkg):
    """inputs of A (folded launches of every load path, sps, freq_shift and burst type), B (peaks at tile edges, ragged last
    tiles), C (launch geometry, and a sequence that grows, shrinks and reshapes the fold buffer) and D (folded rough_multi)"""
    rng = np.random.default_rng(4242)
    C = []
    ns = 93600
    # A: folded launches (> 512 work-groups)
    for sps, n in ((1, 12), (2, 23), (8, 86), (16, 172)):
        L = ns if sps <= 2 else ns * sps // 8                  # 46 / 23 / 6 / 6 tiles
        C.append(_rough_case("A sps %d" % sps, _clear_windows(pkg, rng, 8, L, sps), n, L, sps))
    dc = [0, 7.0 - 3.0j, -40.0 + 25.0j, 0, 3.0 + 11.0j, 0, 0.02j, 0]
    C.append(_rough_case("A sps 4 odd length, dc", _clear_windows(pkg, rng, 8, ns + 1, 4, dc=dc), 44, ns + 1, 4))
    C.append(_rough_case("A sps 4 odd offsets", _clear_windows(pkg, rng, 8, ns + 3, 4), 44, ns + 3, 4, odd=True))
    fs = [0.0, 0.05, -0.05, 0.0, 0.013, -0.031, 0.0, 0.05]
    C.append(_rough_case("A freq_shift", _clear_windows(pkg, rng, 8, ns, 4, fs=fs), 44, ns, 4, fs=fs))
    for which in ("fcch3_lband", "fcch3_sband"):
        C.append(_rough_case("A " + which, _clear_windows(pkg, rng, 6, ns, 4, which), 44, ns, 4, which))
    # B: the best window at m0 + 2040 ... m0 + 2044 of interior tiles 3, 4 and 5 (each of them gives up under one of the
    # FOLD_GIVEUP modes while its successor folds), 12 tiles a stream
    targets = [t * TILE_STEP + 2040 + d for t in (3, 4, 5) for d in range(5)]
    C.append(_rough_case("B tile edges", _edge_windows(pkg, rng, ns, 4, targets), 45, ns, 4, want=targets))
    # B: ragged last tiles, nlags = 11 * 2044 + j: the last tile holds 1 ... 4 lags, all of them in the previous tile's windows
    for j in (1, 2, 3, 4):
        nl = 11 * TILE_STEP + j
        L = 4 * (nl + 116) + 2
        wins = _edge_windows(pkg, rng, L, 4, [nl - 5, nl - 6]) + _clear_windows(pkg, rng, 2, L, 4)
        C.append(_rough_case("B ragged %d" % j, wins, 43, L, 4, want=[nl - 5, nl - 6, None, None]))
    # C: geometry -- 512 work-groups (two-kernel form, pick inside k_fcch_energy) and 513 (folded); 64 tiles a stream (folded)
    # and 65 (two-kernel); 4 104 (four lag tiles per k_fcch_energy work-group)
    L8 = 4 * (8 * TILE_STEP - 300 + 116)
    C.append(_rough_case("C 8 x 64 = 512", _clear_windows(pkg, rng, 8, L8, 4), 64, L8, 4))
    L9 = 4 * (9 * TILE_STEP - 700 + 116)
    C.append(_rough_case("C 9 x 57 = 513", _clear_windows(pkg, rng, 8, L9, 4), 57, L9, 4))
    L64 = 4 * (64 * TILE_STEP + 116)
    w64 = _clear_windows(pkg, rng, 3, L64 + 4, 4)
    C.append(_rough_case("C 64 tiles", [x[:L64] for x in w64], 9, L64, 4))
    C.append(_rough_case("C 65 tiles", w64, 8, L64 + 4, 4))
    C.append(_rough_case("C 12 x 342 = 4104", _clear_windows(pkg, rng, 16, ns, 4), 342, ns, 4))
    # C: one process, a sequence whose record count grows past the fold buffer, shrinks and changes shape
    w = _clear_windows(pkg, rng, 8, ns, 4)
    for name, n in (("C seq 516", 43), ("C seq 6 000", 500), ("C seq 516 again", 43)):
        C.append(_rough_case(name, w, n, ns, 4))
    w1 = _clear_windows(pkg, rng, 4, 50000, 1)
    C.append(_rough_case("C seq sps 1, 25 tiles", w1, 30, 50000, 1))
    C.append(_rough_case("C seq 64 tiles x 150", [x[:L64] for x in w64], 150, L64, 4))
    C.append(_rough_case("C seq 516 last", w, 43, ns, 4))
    # D: folded rough_multi (65 windows of 60 840 samples, 8 tiles each), with and without freq_shift; and at 2 samples a
    # symbol (15 lag tiles, 8 statistics spans)
    for name, sps, n, with_fs in (("D multi", 4, 65, False), ("D multi freq_shift", 4, 65, True), ("D multi sps 2", 2, 35, False)):
        L = 60840
        wins = []
        for i in range(n):
            s, _ = pkg.synth.synth_fcch_stream(L, sps, rng, snr_db=6.0, cfo_hz=float(rng.uniform(-300, 300)),
                                               first=int(rng.integers(200, 5000)))
            for extra in range(i % 3):
                s2, _ = pkg.synth.synth_fcch_stream(L, sps, rng, snr_db=3.0, cfo_hz=float(rng.uniform(-300, 300)),
                                                    first=int(rng.integers(8000, 25000)))
                s = s + np.complex64(0.7) * s2
            wins.append(s.astype(np.complex64))
        c = _rough_case(name, wins, n, L, sps, fs=rng.choice([0.0, 0.02, -0.04], n) if with_fs else None)
        c["kind"] = "multi"
        C.append(c)
    return C


def run_cases(api, cases):
    out = []
    for c in cases:
        if c["kind"] == "rough":
            toa, rv = api.fcch_rough_batch(c["iq"], c["off"], c["len"], sps=c["sps"], freq_shift=c["fs"], fcch_type=c["which"])
            out.append(dict(toa=[int(t) for t in toa], rv=[int(r) for r in rv]))
        else:
            cnt, toa = api.fcch_rough_multi_batch(c["iq"], c["off"], c["len"], sps=c["sps"], freq_shift=c["fs"], N=16)
            out.append(dict(cnt=[int(v) for v in cnt], toa=[[int(t) for t in toa[i, :max(int(cnt[i]), 0)]]
                                                            for i in range(len(cnt))]))
    return out


def oracle_results(orc, c):
    """the oracle's answer per stream (computed once per distinct window and freq_shift)"""
    memo, out = {}, []
    for i, o in enumerate(c["off"]):
        f = 0.0 if c["fs"] is None else float(c["fs"][i])
        key = (int(o), f)
        if key not in memo:
            x = c["iq"][int(o):int(o) + c["len"]]
            if c["kind"] == "rough":
                memo[key] = orc.fcch_rough(x, c["sps"], f, which=c["which"])
            else:
                rv, t = orc.fcch_rough_multi(x, c["sps"], f, N=16)
                memo[key] = (rv, [int(v) for v in t])
        out.append(memo[key])
    return out


def check(c, got, want):
    if c["kind"] == "rough":
        assert all(w[0] == 0 for w in want), c["name"]
        assert got["rv"] == [0] * len(want), (c["name"], got["rv"])
        bad = [(i, got["toa"][i], w[1]) for i, w in enumerate(want) if got["toa"][i] != w[1]]
        assert not bad, (c["name"], "stream, toa, oracle toa", bad[:8], len(bad))
    else:
        assert got["cnt"] == [w[0] for w in want], (c["name"], got["cnt"], [w[0] for w in want])
        bad = [i for i, w in enumerate(want) if got["toa"][i] != w[1]]
        assert not bad, (c["name"], [(i, got["toa"][i], want[i][1]) for i in bad[:4]], len(bad))
        assert min(w[0] for w in want) >= 1


@pytest.fixture(scope="module")
def cases(pkg, orc):
    cs = build_cases(pkg)
    for c in cs:
        c["oracle"] = oracle_results(orc, c)
        if c["kind"] == "rough":
            for w, o in enumerate(c["woff"]):
                fs = 0.0 if c["fs"] is None else float(c["fs"][w])
                assert _clear(c["iq"][int(o):int(o) + c["len"]], c["sps"], fs, c["which"])[0], (c["name"], w)
        for w, t in enumerate(c["want"] or []):
            if t is not None:
                # the intended window, by a clear margin (float64), and the oracle agrees on the toa it implies
                ok, best, margin = _clear(c["iq"][int(c["woff"][w]):int(c["woff"][w]) + c["len"]], c["sps"], want=t)
                assert ok and best == t and margin > 1e-3, (c["name"], w, best, t, margin)
    return cs


def test_folded_sweep_matches_oracle(gpu_api, cases):
    """A-D on the product build: every launch of more than 512 work-groups folded, the rest in the two-kernel form."""
    got = run_cases(gpu_api, cases)
    for c, g in zip(cases, got):
        check(c, g, c["oracle"])


def test_tile_edge_peaks_are_where_intended(cases):
    """B's windows: the peak of the oracle's choice sits at the intended lag (m0 + 2040 ... m0 + 2044, the last lags of a
    ragged stream), i.e. the edge cases are the ones asked for and not shifted into a tile's interior."""
    for c in cases:
        if c["want"] is None:
            continue
        for w, t in enumerate(c["want"]):
            if t is not None:
                i = w                                             # stream w reads window w
                assert abs(c["oracle"][i][1] / c["sps"] - (t + 2)) <= 2.5, (c["name"], w, c["oracle"][i][1], t)


def _child_main(f_in, f_out):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.api.load()
    pkg.api.init(0)
    meta = json.load(open(f_in + ".json"))
    data = np.load(f_in + ".npz")
    cases = []
    for k, m in enumerate(meta):
        c = dict(m, iq=data["iq%d" % k], off=data["off%d" % k], fs=data["fs%d" % k] if m["has_fs"] else None)
        cases.append(c)
    json.dump(run_cases(pkg.api, cases), open(f_out, "w"))


MODES = [
    {"GMR1_HIP_FCCH_FOLD_POLLS": "0"},                     # every tile gives up
    {"GMR1_HIP_FCCH_FOLD_GIVEUP": "2,0"},                  # some tiles of a stream fold, their neighbours give up
    {"GMR1_HIP_FCCH_FOLD_GIVEUP": "2,1"},
    {"GMR1_HIP_FCCH_FOLD_GIVEUP": "3,2"},
    {"GMR1_HIP_FCCH_FOLD_GIVEUP": "64,-1"},                # the stream's last tile only
    {"GMR1_HIP_FCCH_UNFOLDED": "1"},                       # the two-kernel form at every size
    {"GMR1_HIP_FCCH_TWO_PASS": "1"},                       # k_fcch_stats + k_fcch_corr
]


def test_folded_fallbacks_profiling_build(cases, tmp_path):
    """A-D in a child process per fallback mode on the profiling build, the sweep's scratch poisoned: identical to the oracle."""
    if not os.path.exists(PROF):
        pytest.skip("the profiling build (python osmo-gmr_amd/build.py --profile) is not there")
    f_in = str(tmp_path / "fold_cases")
    np.savez(f_in + ".npz", **{k: v for i, c in enumerate(cases)
                               for k, v in (("iq%d" % i, c["iq"]), ("off%d" % i, c["off"]),
                                            ("fs%d" % i, c["fs"] if c["fs"] is not None else np.zeros(0, np.float32)))})
    json.dump([dict(name=c["name"], kind=c["kind"], len=c["len"], sps=c["sps"], which=c["which"], has_fs=c["fs"] is not None)
               for c in cases], open(f_in + ".json", "w"))
    code = "import sys; sys.path.insert(0, %r); import test_gpu_fcch_fold as t; t._child_main(%r, sys.argv[1])" % (
        os.path.join(ROOT, "tests"), f_in)
    for mode in MODES:
        env = dict(os.environ, GMR1_HIP_LIBRARY=PROF, GMR1_HIP_FCCH_POISON="1", **mode)
        f_out = str(tmp_path / "fold_out.json")
        r = subprocess.run([sys.executable, "-c", code, f_out], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-2000:])          # (the loop stops at the first failing child)
        got = json.load(open(f_out))
        for c, g in zip(cases, got):
            try:
                check(c, g, c["oracle"])
            except AssertionError as e:
                raise AssertionError("%s: %s" % (mode, e)) from None
