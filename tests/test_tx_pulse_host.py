"""The shaped modulator (gmr1_hip_shape_batch*, gmr1_hip_mod_shaped_batch*) without a GPU: the pulse and the index rule
the kernel runs (osmo-gmr_amd/csrc/tx_pulse.h), compiled for the host as a stand-alone program, plain and under
-fsanitize=address,undefined, against synth.rc_pulse / rrc_pulse / shape_bursts; the four entries are declared, exported and
mirrored; every bad argument is refused before the device is asked for and leaves the output alone; and without a device the
calls say so."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_shape_batch_dev", "gmr1_hip_shape_batch", "gmr1_hip_mod_shaped_batch_dev", "gmr1_hip_mod_shaped_batch")
EINVAL, ENODEV = 22, 19
ALPHA = 0.35
SPS = (1, 2, 3, 4, 5, 8, 16)
SPANS = (1, 5, 8)


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:       # noqa: BLE001 - no torch, no device either
        return True


# ---- tx_pulse.h on the host ----
def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "tx_pulse_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("txpulse"), "tx_pulse_host", [])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("txpulsesan"), "tx_pulse_host_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout
    out = out.split("\n")
    assert len(out) == len(lines) + 1 and out[-1] == ""
    return out[:-1]


def _floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def _pulse(synth, pulse):
    return synth.rrc_pulse if pulse else synth.rc_pulse


def _within_one_ulp(got, want64):
    """got (float32) against want64 rounded to float32: at most one float32 ulp apart"""
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))


def _fracs():
    rng = np.random.default_rng(350)
    return np.concatenate([[0.0, 0.5, -0.5, 0.25], rng.uniform(-0.5, 0.5, 36)]).astype(np.float32).astype(np.float64)


def _check_pulses(exe, synth):
    # the coefficient tables: t = m + (p - frac) / sps for every m, p
    cases = [(pulse, sps, span, fr) for pulse in (0, 1) for sps in SPS for span in SPANS for fr in _fracs()]
    lines = _run(exe, ["C %d %d %d %.17g" % c for c in cases])
    worst = 0
    for (pulse, sps, span, fr), ln in zip(cases, lines):
        w = ln.split()
        assert int(w[0]) == (2 * span + 1) * sps == len(w) - 1
        got = _floats(w[1:]).reshape(2 * span + 1, sps)
        m = np.arange(-span, span + 1, dtype=np.float64)[:, None]
        p = np.arange(sps, dtype=np.float64)[None, :]
        want = _pulse(synth, pulse)(m + (p - fr) / sps)
        ok = _within_one_ulp(got, want)
        assert ok.all(), (pulse, sps, span, fr, got[~ok], want[~ok])
        worst += int((got != want.astype(np.float32)).sum())
    # the singular points and their neighbourhoods on both sides of the switch thresholds
    pts = [0.0, 1e-10, -1e-10, 1e-8, -1e-8]
    for t0 in (1 / (2 * ALPHA), 1 / (4 * ALPHA)):
        for sign in (1, -1):
            pts += [sign * t0, sign * t0 * (1 + 1e-12), sign * t0 * (1 - 1e-12), sign * (t0 + 1e-7), sign * (t0 - 1e-7)]
    for pulse in (0, 1):
        got = _floats(_run(exe, ["T %d %.17g" % (pulse, t) for t in pts]))
        want = _pulse(synth, pulse)(np.array(pts))
        ok = _within_one_ulp(got, want)
        assert ok.all(), (pulse, np.array(pts)[~ok], got[~ok], want[~ok])
    assert _floats(_run(exe, ["T 0 0"]))[0] == 1.0
    assert _floats(_run(exe, ["T 1 0"]))[0] == np.float32(1 - ALPHA + 4 * ALPHA / np.pi)
    assert _floats(_run(exe, ["T 0 %.17g" % (1 / (2 * ALPHA))]))[0] == np.float32(np.pi / 4 * np.sinc(1 / (2 * ALPHA)))
    return worst


def _restated_index(start, span, sps, length, in_len):
    k = np.arange(in_len, dtype=np.int64)
    q = k - (start - span * sps)
    return np.where((q >= 0) & (q < (length + 2 * span) * sps), q, -1)


def _window_cases():
    """(start, span, sps, len, in_len): the body inside, clipped on the left, on the right, on both sides (in_len shorter
    than the body), wholly outside on either side, and starts at the ends of int32"""
    out = []
    for sps in (1, 3, 4, 16):
        for span in (1, 5, 8):
            length = 7
            body = (length + 2 * span) * sps
            for start, in_len in ((span * sps + 2, body + 5), (span * sps, body), (-3 * sps, body), (0, body),
                                  (body - 2 * sps, body), (span * sps, body - 3 * sps - 1), (-2 * sps, 5), (2, 1),
                                  (-body - 5, 9), (-(length + span) * sps, 4), (-(length + span) * sps + 1, 4),
                                  (9 + span * sps, 9), (8 + span * sps, 9), (2 ** 31 - 1, 6), (-2 ** 31, 6)):
                out.append((start, span, sps, length, in_len))
    # the longest body there is, at every sps: q div sps over its whole range
    out += [(8 * sps + 1, 8, sps, 2048, (2048 + 16) * sps + 3) for sps in range(1, 17)]
    return out


def _check_index_rule(exe):
    cases = _window_cases()
    lines = _run(exe, ["W %d %d %d %d %d" % c for c in cases])
    seen = set()
    for c, ln in zip(cases, lines):
        got = np.array(ln.split(), np.int64)
        want = _restated_index(*c)
        assert np.array_equal(got, want), c
        inside = want >= 0
        seen.add((bool(inside[0]), bool(inside[-1]), bool(inside.any())))
    # inside with zeros on both sides, clipped left, clipped right, clipped on both sides, nothing written
    assert seen == {(False, False, True), (True, False, True), (False, True, True), (True, True, True), (False, False, False)}


def _check_body(exe, synth):
    """The window the rule and the taps give, without rotation and gain, against synth.shape_bursts put at `start`"""
    rng = np.random.default_rng(77)
    for pulse, sps, span, length, start, in_len in ((0, 4, 5, 9, 22, 80), (1, 3, 8, 5, -7, 40), (0, 1, 1, 6, 2, 10),
                                                   (1, 16, 3, 4, 100, 150), (0, 5, 8, 3, -30, 200)):
        fr = float(np.float32(rng.uniform(-0.5, 0.5)))
        sym = (rng.standard_normal(length) + 1j * rng.standard_normal(length)).astype(np.complex64)
        line = "S %d %d %d %.17g %d %d %d " % (pulse, sps, span, fr, start, in_len, length)
        line += " ".join("%.9g %.9g" % (s.real, s.imag) for s in sym)
        got = _floats(_run(exe, [line])[0].split()).view(np.complex64)
        body = synth.shape_bursts(sym[None, :], sps, fr, span, "rrc" if pulse else "rc")[0]
        want = np.zeros(in_len, np.complex64)
        s0 = start - span * sps
        lo, hi = max(0, s0), min(in_len, s0 + body.size)
        if hi > lo:
            want[lo:hi] = body[lo - s0:hi - s0]
        m = np.arange(-span, span + 1)[:, None]
        g = np.abs(_pulse(synth, pulse)(m + (np.arange(sps)[None, :] - fr) / sps)).sum(0).max()
        bound = 2.0 ** -23 * (2 * span + 4) * g * np.abs(sym).max()
        assert np.abs(got - want).max() <= bound, (pulse, sps, span)
        assert np.array_equal(got == 0, want == 0)


def _check_args_rule(exe):
    good = dict(n=3, len=117, sps=4, pulse=0, span=5, in_len=484)
    order = ("n", "len", "sps", "pulse", "span", "in_len")
    bad = [dict(n=-1), dict(len=0), dict(len=2049), dict(sps=0), dict(sps=17), dict(pulse=2), dict(pulse=-1), dict(span=0),
           dict(span=9), dict(in_len=0)]
    fine = [dict(), dict(n=0), dict(len=1), dict(len=2048), dict(sps=1), dict(sps=16), dict(pulse=1), dict(span=1), dict(span=8),
            dict(in_len=1)]
    lines = _run(exe, ["A " + " ".join(str(dict(good, **c)[k]) for k in order) for c in bad + fine])
    assert [int(l) for l in lines] == [1] * len(bad) + [0] * len(fine)


def test_pulses_equal_synth_to_one_ulp(program, pkg):
    differing = _check_pulses(program, pkg.synth)
    print("coefficients that are not the float32 of synth's value: %d" % differing)


def test_index_rule_clips_at_both_ends(program):
    _check_index_rule(program)
    _check_args_rule(program)


def test_body_equals_shape_bursts(program, pkg):
    _check_body(program, pkg.synth)


def test_rule_is_clean_under_asan_and_ubsan(program_sanitized, pkg):
    """The same checks on the program built with -fsanitize=address,undefined (a stand-alone host program)."""
    _check_index_rule(program_sanitized)
    _check_args_rule(program_sanitized)
    _check_body(program_sanitized, pkg.synth)


# ---- the entries ----
def test_header_declares_the_calls(pkg):
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert re.search(r"GMR1_HIP_PULSE_RC\s*=\s*0\s*,\s*GMR1_HIP_PULSE_RRC\s*=\s*1", txt)
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    api = pkg.api
    lib = api.load()
    for name in NAMES:
        assert name in table, name
        assert hasattr(lib, name) and name in api.SIGNATURES, name
    assert (api.PULSE_RC, api.PULSE_RRC) == (0, 1)
    for name in ("shape_batch", "mod_shaped_batch", "shape_batch_dev", "mod_shaped_batch_dev"):
        assert callable(getattr(api, name)), name


SENT = np.float32(-7.25)


def _shape_args():
    """A well-formed three-burst call over host arrays, out filled with a guard value"""
    rng = np.random.default_rng(5)
    n, length, in_len = 3, 12, 64
    return dict(sym=(rng.standard_normal((n, length * 2))).astype(np.float32), eb=rng.integers(0, 2, (n, 208), dtype=np.uint8),
                sid=np.array([0, 1, 0], np.int32), off=np.array([0, 70, 140], np.uint64),
                start=np.full(n, 8, np.int32), frac=np.zeros(n, np.float32), cfo=np.zeros(n, np.float32),
                ph=np.zeros(n, np.float32), gain=np.ones(n, np.float32), out=np.full(2 * 210, SENT, np.float32))


def _calls(api, a):
    p = lambda k: a[k].ctypes.data
    shape_good = dict(n=3, len=12, sps=4, pulse=0, span=2, in_len=64, src=p("sym"), off=p("off"), start=p("start"),
                      frac=p("frac"), cfo=p("cfo"), ph=p("ph"), gain=p("gain"), out=p("out"), out_len=210)
    # nt3_facch: 104 burst bits, two training sequences, 117 symbols
    mod_good = dict(shape_good, burst=5, sps=1, in_len=60, sid=p("sid"), src=p("eb"))
    sh_dev, sh, ms_dev, ms = (api._fn(nm) for nm in NAMES)

    def shape(dev):
        def f(n, len, sps, pulse, span, in_len, src, off, start, frac, cfo, ph, gain, out, out_len):
            args = (n, len, sps, pulse, span, in_len, src, off, start, frac, cfo, ph, gain, out, out_len)
            return sh_dev(None, *args) if dev else sh(*args)
        return f

    def mod(dev):
        def f(burst, n, len, sps, pulse, span, in_len, src, sid, off, start, frac, cfo, ph, gain, out, out_len):
            args = (burst, n, sps, pulse, span, in_len, src, sid, off, start, frac, cfo, ph, gain, out, out_len)
            return ms_dev(None, *args) if dev else ms(*args)
        return f

    return (shape_good, shape(True), shape(False)), (mod_good, mod(True), mod(False))


BAD_BOTH = [dict(sps=0), dict(sps=17), dict(sps=-4), dict(span=0), dict(span=9), dict(pulse=2), dict(pulse=-1), dict(in_len=0),
            dict(in_len=-5), dict(n=-1), dict(src=None), dict(off=None), dict(out=None)]


def test_bad_arguments_are_refused_and_nothing_is_written(pkg):
    api = pkg.api
    a = _shape_args()
    keep = a["out"].tobytes()
    (sg, s_dev, s_host), (mg, m_dev, m_host) = _calls(api, a)
    for good, dev, host, extra, who in ((sg, s_dev, s_host, [dict(len=0), dict(len=2049), dict(len=-1)], b"shape_batch"),
                                        (mg, m_dev, m_host, [dict(burst=-1), dict(burst=10)], b"mod_shaped_batch")):
        for f in (dev, host):
            for change in BAD_BOTH + extra:
                assert f(**dict(good, **change)) == -EINVAL, change
                assert who in api._fn("gmr1_hip_last_error")()
        # the host forms see the arrays: a window that leaves out, windows that overlap
        assert host(**dict(good, out_len=int(a["off"][2]) + good["in_len"] - 1)) == -EINVAL
        assert host(**dict(good, out_len=0)) == -EINVAL
        was = a["off"].copy()
        for off in ([0, good["in_len"] - 1, 140], [140, 0, 100], [5, 5, 140], [0, 70, 2 ** 64 - 1]):
            a["off"][:] = np.array(off, np.uint64)
            assert host(**good) == -EINVAL, off
        a["off"][:] = was
    # a training sequence the format does not have
    for sid in ([0, 2, 0], [-1, 0, 0], [0, 0, 2 ** 31 - 1]):
        a["sid"][:] = sid
        assert m_host(**mg) == -EINVAL, sid
    a["sid"][:] = [0, 1, 0]
    bcch = dict(mg, burst=0, sid=a["sid"].ctypes.data)          # one sequence only
    assert m_host(**bcch) == -EINVAL
    assert a["out"].tobytes() == keep


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_the_calls_say_so(pkg):
    api = pkg.api
    a = _shape_args()
    keep = a["out"].tobytes()
    for good, dev, host in _calls(api, a):
        for f in (dev, host):
            assert f(**good) == -ENODEV
            assert f(**dict(good, start=None, frac=None, cfo=None, ph=None, gain=None)) == -ENODEV
            assert f(**dict(good, n=0)) == -ENODEV
            assert f(**dict(good, n=-1)) == -EINVAL              # bad arguments come first
    assert a["out"].tobytes() == keep
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.shape_batch(np.ones((2, 5), np.complex64), 4, 60)
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.mod_shaped_batch("bcch", np.zeros((2, 424), np.uint8), 4, 500, sync_id=0)
