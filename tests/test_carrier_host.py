"""The carrier mixer and the FCCH chirp windows (gmr1_hip_carrier_mix*, gmr1_hip_fcch_chirp_batch*) without a GPU.

1. The noise rule the kernel runs (osmo-gmr_amd/csrc/carrier_noise.h), compiled for the host as a stand-alone program
   (tests/c/carrier_noise_host.cpp), plain and under -fsanitize=address,undefined: the Random123 known answers of
   Philox4x32-10; words and uniforms equal to the numpy restatement (tests/carrier_ref.py) exactly, z within float rounding;
   the carrier phase at indices past 2^33 against extended precision.
2. The restatement's own statistics on 2^20 samples: a property of the rule, checked once here.
3. Every refusal of the four entries, before the device is asked for and with the output untouched; without a device the
   calls say so.
4. The closed-loop inputs (tests/carrier_cases.py): the oracle's receive loop on the float64 restatement alone finds what
   tests/test_gpu_carrier.py then asks of the device chain, so that test cannot hide behind its inputs."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import carrier_cases as cc
import carrier_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_fcch_chirp_batch_dev", "gmr1_hip_fcch_chirp_batch", "gmr1_hip_carrier_mix_dev", "gmr1_hip_carrier_mix")
EINVAL, ENODEV = 22, 19


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:       # noqa: BLE001 - no torch, no device either
        return True


# ---- carrier_noise.h on the host ----
def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "carrier_noise_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cnoise"), "carrier_noise_host", [])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cnoisesan"), "carrier_noise_host_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout
    out = out.split("\n")
    assert len(out) == len(lines) + 1 and out[-1] == ""
    return out[:-1]


# counter, key -> words: the Random123 known-answer vectors of philox4x32_10
KAT = [("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _check_known_answers(exe):
    assert _run(exe, ["P %s %s" % (c, k) for c, k, _ in KAT]) == [w for _, _, w in KAT]
    for c, k, w in KAT:           # and the restatement gives them too
        got = ref.philox4x32_10(np.array([int(x, 16) for x in c.split()]), np.array([int(x, 16) for x in k.split()]))
        assert ["%08x" % int(v) for v in got] == w.split()


# (seed, noise id, first sample, count): both parities of first, a negative start, indices whose pair counter needs its high word
NOISE_RUNS = [(0, 0, 0, 1024), (cc.SEED, 3, 1, 1023), (2 ** 64 - 1, 2 ** 32 - 1, -5, 64), (12345, 7, 2 ** 33 + 1, 512),
              (12345, 8, 2 ** 40 - 3, 64)]


def _check_noise(exe):
    lines = _run(exe, ["N %d %d %d %d" % r for r in NOISE_RUNS])
    worst = 0.0
    for (seed, nid, first, count), ln in zip(NOISE_RUNS, lines):
        w = np.array([int(x, 16) for x in ln.split()], np.uint32).reshape(count, 6)
        n = first + np.arange(count, dtype=np.int64)
        wa, wb = ref.noise_words(seed, nid, n)
        assert np.array_equal(w[:, 0], wa) and np.array_equal(w[:, 1], wb), (seed, nid, first)
        u1, u2 = ref.uniforms(wa, wb)
        assert np.array_equal(w[:, 2].view(np.float32).astype(np.float64), u1)         # exact: multiples of 2^-24
        assert np.array_equal(w[:, 3].view(np.float32).astype(np.float64), u2)
        assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
        z, r = ref.noise(seed, nid, n)
        got = w[:, 4].view(np.float32).astype(np.float64) + 1j * w[:, 5].view(np.float32).astype(np.float64)
        # libm's logf / sqrtf and a cos / sin through double: a few float roundings of r and of the unit vector
        err = np.abs(got - z) / (2.0 ** -23 * (4.0 * r + 1.0))
        worst = max(worst, err.max())
        assert (err <= 1.0).all(), (seed, nid, first, err.max())
    return worst


PHASES = [(2 * np.pi * 120.0 / 93600.0, n) for n in (0, 1, 2 ** 23 + 1, 2 ** 33, 2 ** 33 + 1, 2 ** 33 + 70001, -(2 ** 33) - 7)]
PHASES += [(-2 * np.pi * 300.0 / 93600.0, 2 ** 33 + 12345), (0.5, 2 ** 40 + 1), (3.0, 2 ** 31 - 1)]


def _check_phase(exe):
    got = np.array([int(x, 16) for x in _run(exe, ["F %.17g %d" % p for p in PHASES])], np.uint32).view(np.float32)
    for (cfo, n), g in zip(PHASES, got):
        want, turns = ref.phase(cfo, np.array([n]))
        # the product's rounding in double (2^-53 |cfo n|, doubled for the two-part 2 pi), the rounding to float of a value
        # of at most pi (half an ulp of [2, 4): 2^-23); compared modulo 2 pi, since -pi and pi are the same phase
        d = abs(float(g) - want[0])
        d = min(d, abs(d - 2 * np.pi))
        assert d <= 2.0 ** -23 + 2.0 ** -52 * turns[0], (cfo, n, float(g), want[0])
        assert abs(float(g)) <= np.float32(np.pi) + np.float32(2.0 ** -22)
    # what a float phase would have given at 2^33: wrong by radians, not by roundings
    cfo, n = PHASES[3]
    f32 = np.float32(cfo) * np.float32(n)
    want, _ = ref.phase(cfo, np.array([n]))
    assert abs(np.angle(np.exp(1j * (float(f32) - want[0])))) > 0.05


def test_philox_known_answers(program):
    _check_known_answers(program)


def test_noise_rule_equals_the_restatement(program):
    worst = _check_noise(program)
    print("worst |z - restatement| over its bound: %.3f" % worst)


def test_carrier_phase_past_2_to_the_33(program):
    _check_phase(program)


def test_rule_is_clean_under_asan_and_ubsan(program_sanitized):
    """The same checks on the program built with -fsanitize=address,undefined (a stand-alone host program)."""
    _check_known_answers(program_sanitized)
    _check_noise(program_sanitized)
    _check_phase(program_sanitized)


def test_noise_statistics_of_the_rule():
    """2^20 samples of one stream under a fixed seed: mean, variance per component, I/Q correlation and lag-1 autocorrelation
    within 5 standard errors of 0, 1, 0, 0.  With N samples of a unit Gaussian the standard errors are 1 / sqrt(N) for a
    mean or a correlation of independent components and sqrt(2 / N) for a variance."""
    N = 1 << 20
    z, _ = ref.noise(cc.SEED, 1, np.arange(N, dtype=np.int64))
    se = 1.0 / np.sqrt(N)
    for comp in (z.real, z.imag):
        assert abs(comp.mean()) <= 5 * se, comp.mean()
        assert abs(comp.var() - 1.0) <= 5 * np.sqrt(2.0) * se, comp.var()
        assert abs(np.mean(comp[:-1] * comp[1:])) <= 5 * se
    assert abs(np.mean(z.real * z.imag)) <= 5 * se
    assert abs(np.mean(z.real[:-1] * z.imag[1:])) <= 5 * se and abs(np.mean(z.imag[:-1] * z.real[1:])) <= 5 * se
    # another stream, another seed: other samples
    z2, _ = ref.noise(cc.SEED, 2, np.arange(64, dtype=np.int64))
    z3, _ = ref.noise(cc.SEED + 1, 1, np.arange(64, dtype=np.int64))
    assert not np.array_equal(z2, z[:64]) and not np.array_equal(z3, z[:64])


# ---- the entries ----
def test_header_declares_the_calls(pkg):
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert "gmr1_hip_carrier_mix" in txt.split("a caller who wants noise")[1][:300]
    assert re.search(r"#define\s+GMR1_HIP_CARRIER_MIX_TILE\s+%d\b" % pkg.api.CARRIER_MIX_TILE, txt)
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    api = pkg.api
    lib = api.load()
    for name in NAMES:
        assert name in table, name
        assert hasattr(lib, name) and name in api.SIGNATURES, name
    for name in ("fcch_chirp_batch", "fcch_chirp_batch_dev", "carrier_mix", "carrier_mix_dev"):
        assert callable(getattr(api, name)), name


SENT = np.float32(-7.25)


def _chirp_args():
    return dict(off=np.array([0, 500, 1000], np.uint64), start=np.zeros(3, np.int32), frac=np.zeros(3, np.float32),
                cfo=np.zeros(3, np.float32), ph=np.zeros(3, np.float32), gain=np.ones(3, np.float32),
                out=np.full(2 * 1500, SENT, np.float32))


def _chirp_calls(api, a):
    p = lambda k: a[k].ctypes.data
    good = dict(fcch_type=0, n=3, sps=4, in_len=468, off=p("off"), start=p("start"), frac=p("frac"), cfo=p("cfo"), ph=p("ph"),
                gain=p("gain"), out=p("out"), out_len=1500)
    f_dev, f_host = api._fn(NAMES[0]), api._fn(NAMES[1])
    order = ("fcch_type", "n", "sps", "in_len", "off", "start", "frac", "cfo", "ph", "gain", "out", "out_len")
    dev = lambda **kw: f_dev(None, *[kw[k] for k in order])
    host = lambda **kw: f_host(*[kw[k] for k in order])
    return good, dev, host


def _mix_args():
    """Two carriers, three segments, out filled with a guard value"""
    return dict(iq=np.ones(2 * 100, np.float32), sf=np.array([0, 2, 3], np.int32), src=np.array([0, 30, 60], np.uint64),
                pos=np.array([5, 5, -3], np.int64), ln=np.array([30, 30, 40], np.uint32), off=np.array([0, 70], np.uint64),
                length=np.array([64, 50], np.uint64), first=np.zeros(2, np.int64), sigma=np.array([0.5, 0.0], np.float32),
                cfo=np.zeros(2, np.float64), nid=np.array([1, 2], np.uint32), out=np.full(2 * 130, SENT, np.float32))


def _mix_calls(api, a):
    p = lambda k: a[k].ctypes.data
    good = dict(n=2, iq=p("iq"), iq_len=100, n_seg=3, sf=p("sf"), src=p("src"), pos=p("pos"), ln=p("ln"), max_seg=40, off=p("off"),
                length=p("length"), max_len=64, first=p("first"), sigma=p("sigma"), cfo=p("cfo"), nid=p("nid"), seed=9, out=p("out"),
                out_len=130)
    f_dev, f_host = api._fn(NAMES[2]), api._fn(NAMES[3])
    dev_order = ("n", "iq", "sf", "src", "pos", "ln", "max_seg", "off", "length", "max_len", "first", "sigma", "cfo", "nid", "seed", "out")
    host_order = ("n", "iq", "iq_len", "n_seg", "sf", "src", "pos", "ln", "max_seg", "off", "length", "max_len", "first", "sigma",
                  "cfo", "nid", "seed", "out", "out_len")
    dev = lambda **kw: f_dev(None, *[kw[k] for k in dev_order])
    host = lambda **kw: f_host(*[kw[k] for k in host_order])
    return good, dev, host


CHIRP_BAD_BOTH = [dict(fcch_type=-1), dict(fcch_type=3), dict(sps=0), dict(sps=17), dict(sps=-4), dict(in_len=0), dict(in_len=-5),
                  dict(n=-1), dict(off=None), dict(out=None)]
MIX_BAD_BOTH = [dict(n=-1), dict(off=None), dict(length=None), dict(out=None), dict(iq=None), dict(src=None), dict(pos=None),
                dict(ln=None), dict(max_seg=0)]


def _set(a, key, values):
    was = a[key].copy()
    a[key][:] = values
    return was


def test_bad_arguments_are_refused_and_nothing_is_written(pkg):
    api = pkg.api
    err = api._fn("gmr1_hip_last_error")
    # the chirp windows: what shape_batch refuses
    a = _chirp_args()
    keep = a["out"].tobytes()
    good, dev, host = _chirp_calls(api, a)
    for f in (dev, host):
        for change in CHIRP_BAD_BOTH:
            assert f(**dict(good, **change)) == -EINVAL, change
            assert b"fcch_chirp_batch" in err()
    assert host(**dict(good, out_len=1000 + 468 - 1)) == -EINVAL            # a window leaves out
    assert host(**dict(good, out_len=0)) == -EINVAL
    for off in ([0, 467, 1000], [1000, 0, 900], [5, 5, 1000], [0, 500, 2 ** 64 - 1]):      # windows overlap / wrap
        was = _set(a, "off", np.array(off, np.uint64))
        assert host(**good) == -EINVAL, off
        a["off"][:] = was
    assert a["out"].tobytes() == keep
    assert host(**good) in (0, -ENODEV) and dev(**dict(good, n=0)) in (0, -ENODEV)
    # the mixer
    a = _mix_args()
    keep = a["out"].tobytes()
    good, dev, host = _mix_calls(api, a)
    for f in (dev, host):
        for change in MIX_BAD_BOTH:
            assert f(**dict(good, **change)) == -EINVAL, change
            assert b"carrier_mix" in err()
    assert host(**dict(good, n_seg=-1)) == -EINVAL
    assert host(**dict(good, sf=None)) == -EINVAL                           # segments without their lists
    for key, values in (("pos", [5, 4, -3]),                                # not sorted within a carrier
                        ("ln", [30, 41, 40]),                               # longer than max_seg_len
                        ("src", [0, 71, 60]), ("src", [0, 30, 2 ** 64 - 1]), ("src", [101, 30, 60]),     # leaves seg_iq
                        ("sf", [1, 2, 3]), ("sf", [0, 2, 2]), ("sf", [0, 2, 4]), ("sf", [0, 3, 2]),      # not 0 .. n_seg, decreasing
                        ("off", [0, 63]), ("off", [70, 30]), ("off", [0, 81]), ("off", [0, 2 ** 64 - 1]),    # overlap, leave out
                        ("length", [65, 50]),                               # more than max_length
                        ("sigma", [-0.5, 0.0]), ("sigma", [np.nan, 0.0]), ("sigma", [0.5, np.inf])):
        was = _set(a, key, values)
        assert host(**good) == -EINVAL, (key, values)
        a[key][:] = was
    assert host(**dict(good, out_len=119)) == -EINVAL and host(**dict(good, iq_len=99)) == -EINVAL
    assert a["out"].tobytes() == keep
    # fine: the same position twice, a segment outside its carrier, no segments at all, nothing to do
    assert host(**good) in (0, -ENODEV)
    assert host(**dict(good, n_seg=0, sf=None, iq=None, src=None, pos=None, ln=None, max_seg=0)) in (0, -ENODEV)
    assert dev(**dict(good, sf=None, iq=None, src=None, pos=None, ln=None, max_seg=0, n=0)) in (0, -ENODEV)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_the_calls_say_so(pkg):
    api = pkg.api
    for args, calls in ((_chirp_args(), _chirp_calls), (_mix_args(), _mix_calls)):
        keep = args["out"].tobytes()
        good, dev, host = calls(api, args)
        for f in (dev, host):
            assert f(**good) == -ENODEV
            assert f(**dict(good, n=0, **({"n_seg": 0, "sf": None} if "n_seg" in good else {}))) == -ENODEV
            assert f(**dict(good, n=-1)) == -EINVAL              # bad arguments come first
        assert args["out"].tobytes() == keep
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.fcch_chirp_batch(2, 4, 468)
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.carrier_mix(np.ones(8, np.complex64), [0, 1], [0], [3], [8], [32], sigma=0.1, cfo=0.01)
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.carrier_mix(None, None, None, None, None, [32, 16], sigma=1.0)


# ---- the closed-loop inputs ----
@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_oracle_reads_the_restated_carrier(pkg, orc, name):
    """The oracle's receive loop on the float64 restatement of each closed-loop case: at least one chain, every BCCH burst
    and all CCCH bursts but at most one of each transmitter it follows, and workloads.match_records' mp == nb, mc >= nc - 1."""
    b = cc.build(pkg, name)
    # the schedule is what the mixer requires: sorted, and on the two-transmitter carrier both transmitters' segments interleave
    assert (np.diff(b["seg_pos"]) >= 0).all() and b["seg_len"].max() <= (cc.BURST_SYMS + 2 * cc.SPAN) * b["sps"]
    assert all(k["n"] >= 3 for k in b["kinds"].values())
    x = cc.restate(pkg, b)
    assert x.size == b["n"] and x.dtype == np.complex64
    orv, rec, chains = orc.rx_run(x, sps=b["sps"], arfcn=0)
    assert orv == 0
    v = cc.check_records(rec, chains, b)
    print(name, "chains", chains, "records", len(rec), v)
    if name == "two_tx":
        assert chains > 1 and len(v) == 4 and all(k[1] for k in v)          # both transmitters are followed
