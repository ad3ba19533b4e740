"""A followed voice call to audio (gmr1_hip_tch3_frames_to_pcm*, gmr1_hip_tch3_voice_batch*) without a GPU: the four
entries are declared, exported and mirrored, every bad argument is refused before the device is asked for and leaves the
output arrays alone, without a device the calls say so -- and the span and classification arithmetic the decoder kernel
runs per call (osmo-gmr_amd/csrc/ambe_calls.h), compiled for the host as a stand-alone program, plain and under
-fsanitize=address,undefined, equals a direct restatement."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tch3_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_tch3_frames_to_pcm_dev", "gmr1_hip_tch3_frames_to_pcm", "gmr1_hip_tch3_voice_batch_dev",
         "gmr1_hip_tch3_voice_batch")
WRAPPERS = ("tch3_frames_to_pcm", "tch3_frames_to_pcm_dev", "tch3_voice", "tch3_voice_dev")
EINVAL, ENODEV = 22, 19


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:       # noqa: BLE001 - no torch, no device either
        return True


def test_header_declares_the_calls():
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    top = txt.split("#ifndef GMR1_HIP_H")[0]                  # the reference-interfaces list
    assert "gmr1_hip_tch3_frames_to_pcm*" in top and "gmr1_hip_tch3_voice_batch*" in top
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in table, name


def test_library_exports_the_symbols_and_the_mirror_has_them(pkg):
    api = pkg.api
    lib = api.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.SIGNATURES, name
    # (restype, arguments...): the _dev forms take the stream first, the host forms flags in front of pcm
    assert len(api.SIGNATURES[NAMES[0]]) == 1 + 8 and len(api.SIGNATURES[NAMES[1]]) == 1 + 8
    assert len(api.SIGNATURES[NAMES[2]]) == 1 + 15 and len(api.SIGNATURES[NAMES[3]]) == 1 + 16
    for name in WRAPPERS:
        assert callable(getattr(api, name)), name


# ---- arguments ----
def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, np.uint8)
    at = -raw.ctypes.data % 16
    return raw[at:at + nbytes]


def records_args(api):
    """A well-formed two-call, three-record invocation over host arrays, the outputs filled with guard values"""
    rec = np.zeros(3, api.TCH3_FRAME)
    rec["type"] = [0x10, 0, 0x10]
    return dict(first=np.array([0, 2, 3], np.int32), rec=rec, cs=_aligned(2 * api.codec_state_bytes(), 0xa5),
                pcm=np.full(3 * 320, 0x5555, np.int16), rv=np.full(6, 7, np.int32))


def records_cases(a):
    p = lambda k: a[k].ctypes.data
    good = dict(n_calls=2, first=p("first"), n_frames=3, frames=p("rec"), cs=p("cs"), flags=0, pcm=p("pcm"), rv=p("rv"))
    bad = [dict(n_calls=-1), dict(n_frames=-1), dict(first=None), dict(frames=None), dict(pcm=None), dict(pcm=p("pcm") + 1),
           dict(cs=p("cs") + 8), dict(cs=p("cs") + 4)]
    return good, bad


def _records_calls(api):
    dev, host = api._fn(NAMES[0]), api._fn(NAMES[1])
    return [lambda n_calls, first, n_frames, frames, cs, flags, pcm, rv: dev(None, n_calls, first, n_frames, frames, cs, pcm, rv),
            lambda n_calls, first, n_frames, frames, cs, flags, pcm, rv: host(n_calls, first, n_frames, frames, cs, flags, pcm, rv)]


def _samples_calls(api):
    dev, host = api._fn(NAMES[2]), api._fn(NAMES[3])
    return [lambda n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out, cs, flags, pcm, rv:
            dev(None, n_calls, sps, in_len, iq, first, n_frames, off, fs, fn, state, out, cs, pcm, rv),
            lambda n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out, cs, flags, pcm, rv:
            host(n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out, cs, flags, pcm, rv)]


def samples_args(api):
    """tch3_cases.call_args (one call, two frames) plus the decoder's arrays, guard-filled"""
    a = tc.call_args(api)
    a.update(cs=_aligned(api.codec_state_bytes(), 0xa5), pcm=np.full(2 * 320, 0x5555, np.int16), rv=np.full(4, 7, np.int32))
    return a


def samples_cases(a):
    good, bad = tc.bad_argument_cases(a)                     # everything the follower refuses
    p = lambda k: a[k].ctypes.data
    good = dict(good, cs=p("cs"), flags=0, pcm=p("pcm"), rv=p("rv"))
    bad = bad + [dict(pcm=None), dict(pcm=p("pcm") + 1), dict(cs=p("cs") + 8)]
    return good, bad


def _outputs(a):
    return b"".join(a[k].tobytes() for k in ("cs", "pcm", "rv") + (("state", "out") if "state" in a else ()))


def test_bad_arguments_are_refused_and_nothing_is_written(pkg):
    api = pkg.api
    for args, cases, calls, who in ((records_args, records_cases, _records_calls, b"tch3_frames_to_pcm"),
                                    (samples_args, samples_cases, _samples_calls, b"tch3_")):
        a = args(api)
        if "state" in a:
            a["state"]["active"] = 1
        keep = _outputs(a)
        good, bad = cases(a)
        dev, host = calls(api)
        for f in (dev, host):
            for change in bad:
                assert f(**dict(good, **change)) == -EINVAL, change
                assert who in api._fn("gmr1_hip_last_error")()
        # the _dev forms need their decoders; the host forms take NULL for fresh ones and have flags
        assert dev(**dict(good, cs=None)) == -EINVAL
        for flags in (4, 8 | api.CODEC_FRESH, -1):
            assert host(**dict(good, flags=flags)) == -EINVAL, flags
        # the host forms see the arrays: a first[] that is not a partition of 0..n_frames
        was = a["first"].copy()
        n = int(was[-1])
        for first in ([1] + list(was[1:]), list(was[:-1]) + [n - 1], list(was[:-1]) + [n + 1]):
            a["first"][:] = first
            assert host(**good) == -EINVAL, first
        a["first"][:] = was
        dec = np.array([0, n, n - 1], np.int32)              # two calls, decreasing
        assert host(**dict(good, n_calls=2, first=dec.ctypes.data, n_frames=n - 1)) == -EINVAL
        if "iq_len" in good:
            assert host(**dict(good, iq_len=1473)) == -EINVAL          # a window that leaves iq
        assert _outputs(a) == keep


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_the_calls_say_so(pkg):
    api = pkg.api
    for args, cases, calls in ((records_args, records_cases, _records_calls), (samples_args, samples_cases, _samples_calls)):
        a = args(api)
        keep = _outputs(a)
        good, _ = cases(a)
        dev, host = calls(api)
        for f in (dev, host):
            assert f(**good) == -ENODEV
            assert f(**dict(good, rv=None)) == -ENODEV
            assert f(**dict(good, n_calls=-1)) == -EINVAL          # bad arguments come first
        for flags in (api.CODEC_FRESH, api.CODEC_CLEARED, api.CODEC_FRESH | api.CODEC_CLEARED):
            assert host(**dict(good, flags=flags)) == -ENODEV
        assert host(**dict(good, cs=None)) == -ENODEV
        assert _outputs(a) == keep
    a = records_args(api)
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.tch3_frames_to_pcm(a["rec"], a["first"])
    b = samples_args(api)
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.tch3_voice(b["iq"], b["first"], b["off"], b["fs"], b["fn"], b["state"])


# ---- ambe_calls.h on the host ----
def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "ambe_calls_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def span_program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ambecalls"), "ambe_calls_host", [])


@pytest.fixture(scope="module")
def span_program_sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ambecallssan"), "ambe_calls_host_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _first_arrays():
    """(n_frames, first): partitions, and arrays with negative entries, entries past n_frames and decreasing entries"""
    rng = np.random.default_rng(2024)
    out = [(0, [0]), (0, [0, 0]), (5, [0, 5]), (5, [5, 0]), (5, [-3, 9]), (5, [9, -3]), (7, [0, 0, 7, 7]),
           (2 ** 31 - 1, [-2 ** 31, 2 ** 31 - 1, 0, 2 ** 31 - 1]), (0, [3, -3, 3])]
    for _ in range(300):
        n_frames = int(rng.choice([0, 1, 2, 63, 64, 65, 1000, 2 ** 31 - 1]))
        n_calls = int(rng.integers(0, 12))
        kind = int(rng.integers(0, 4))
        if kind == 0:          # a partition
            first = np.sort(rng.integers(0, n_frames + 1, n_calls + 1))
            first[0], first[-1] = 0, n_frames
        elif kind == 1:        # anything at all
            first = rng.integers(-2 ** 31, 2 ** 31, n_calls + 1)
        elif kind == 2:        # near the ends, not ordered
            first = rng.integers(-3, n_frames + 4, n_calls + 1)
        else:                  # ordered, but leaving 0..n_frames on both sides
            first = np.sort(rng.integers(-5, n_frames + 6, n_calls + 1))
        out.append((n_frames, [int(x) for x in first]))
    return out


def _restated(n_frames, first):
    """Each of first[c], first[c + 1] clamped to 0..n_frames; where that leaves hi below lo the call is empty at lo"""
    spans = []
    for a, b in zip(first[:-1], first[1:]):
        lo, hi = min(max(a, 0), n_frames), min(max(b, 0), n_frames)
        spans.append((lo, max(hi, lo)))
    return spans


def _check(exe):
    cases = _first_arrays()
    text = "".join("%d %d %s\n" % (n, len(f) - 1, " ".join(map(str, f))) for n, f in cases)
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    head = [int(x) for x in lines[0].split()]
    # the speech test over all 256 values of type: 0x10 alone
    assert head[:256] == [int(t == 0x10) for t in range(256)]
    assert head[256:] == [40, 1, 16, 2, 0x10]
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    assert re.search(r"0x10 two speech frames", txt)
    seen_empty = seen_clamped = 0
    for (n_frames, first), ln in zip(cases, lines[1:]):
        v = [int(x) for x in ln.split()]
        got = list(zip(v[0::2], v[1::2]))
        assert got == _restated(n_frames, first), (n_frames, first)
        for lo, hi in got:
            assert 0 <= lo <= hi <= n_frames, (n_frames, first)
            seen_empty += lo == hi
        seen_clamped += any(x < 0 or x > n_frames for x in first)
        if first and first[0] == 0 and first[-1] == n_frames and first == sorted(first):
            # a partition is tiled: every record belongs to exactly one call
            assert [lo for lo, _ in got] == first[:-1] and [hi for _, hi in got] == first[1:]
    assert len(lines) - 2 == len(cases) and seen_empty and seen_clamped


def test_span_and_speech_test_equal_the_restatement(span_program):
    _check(span_program)


def test_span_is_clean_under_asan_and_ubsan(span_program_sanitized):
    """The same check on the program built with -fsanitize=address,undefined (a stand-alone host program)."""
    _check(span_program_sanitized)
