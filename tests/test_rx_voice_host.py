"""Voice calls to audio in the receive loop (gmr1_hip_tch3_frames_to_audio_dev, gmr1_hip_codec_init_list_dev,
gmr1_hip_rx_run_voice*, gmr1_hip_rx_stream_*voice*) without a GPU: the entries are declared, listed, exported and mirrored;
the block is 656 bytes with its samples at 16; every bad argument is refused before the device is asked for and leaves the
outputs alone; without a device the calls say so -- and the close-up rule the kernels run (osmo-gmr_amd/csrc/tch3_audio.h)
with the loop's carry rule for a chain's assignment count (rx_follow.h), compiled for the host as a stand-alone program,
plain and under -fsanitize=address,undefined, equals a numpy restatement."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rx_voice_cases as vc
import tch3_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_tch3_frames_to_audio_dev", "gmr1_hip_codec_init_list_dev", "gmr1_hip_rx_run_voice_dev", "gmr1_hip_rx_run_voice",
         "gmr1_hip_rx_stream_create_voice", "gmr1_hip_rx_stream_max_audio", "gmr1_hip_rx_stream_push_voice_dev",
         "gmr1_hip_rx_stream_push_voice")
WRAPPERS = ("tch3_frames_to_audio_dev", "tch3_audio_label", "codec_init_list_dev", "rx_run_voice", "rx_run_voice_dev")
EINVAL, ENODEV = 22, 19


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:       # noqa: BLE001 - no torch, no device either
        return True


def test_header_and_integration_table_have_the_calls():
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert re.search(r"struct gmr1_hip_rx_audio \{", txt)
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in table, name


def test_library_exports_the_symbols_and_the_mirror_has_them(pkg):
    api = pkg.api
    lib = api.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.SIGNATURES, name
    want = dict(zip(NAMES, (11, 5, 17, 17, 5, 3, 13, 12)))       # arguments
    for name, n in want.items():
        assert len(api.SIGNATURES[name]) == 1 + n, name
    for name in WRAPPERS:
        assert callable(getattr(api, name)), name
    assert "voice" in api.RxStream.__init__.__code__.co_varnames and callable(api.RxStream.max_audio)


def test_the_block_layout(pkg):
    api = pkg.api
    assert api.RX_AUDIO.itemsize == 656 and api.RX_AUDIO.fields["pcm"][1] == 16
    offs = {k: api.RX_AUDIO.fields[k][1] for k in api.RX_AUDIO.names}
    assert offs == dict(arfcn=0, chain=2, cls=3, fn=4, tn=8, call=9, rv=10, pad=14, pcm=16)
    assert api.tch3_audio_label(0x1234, 0x56, 0x78, 0x9a) == 0x9a78561234
    assert api.tch3_audio_label(0x1ffff, 0x1ff, 0x1ff, 0x1ff) == 0xffffffffff


# ---- arguments ----
def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, np.uint8)
    at = -raw.ctypes.data % 16
    return raw[at:at + nbytes]


def audio_args(api):
    """A well-formed two-call, three-record invocation (host arrays stand in: every refusal comes before they are read)"""
    rec = np.zeros(3, api.TCH3_FRAME)
    rec["type"], rec["cls"] = [0x10, 0, 0x10], [tc.SPEECH, tc.DKAB, tc.SPEECH]
    return dict(first=np.array([0, 2, 3], np.int32), rec=rec, fn=np.arange(3, dtype=np.uint32),
                label=np.array([1, 2], np.uint64), cs=_aligned(2 * api.codec_state_bytes(), 0xa5),
                out=_aligned(3 * 656, 0x5a), n_out=np.full(1, 77, np.int32), call=np.array([0, 1], np.int32))


def _audio_outputs(a):
    return b"".join(a[k].tobytes() for k in ("cs", "out", "n_out"))


def _audio_good(a):
    p = lambda k: a[k].ctypes.data
    return dict(n_calls=2, first=p("first"), n_frames=3, frames=p("rec"), fn=p("fn"), label=p("label"), cs=p("cs"), out=p("out"),
                max_out=3, n_out=p("n_out"))


def _audio_call(api):
    f = api._fn(NAMES[0])
    return lambda n_calls, first, n_frames, frames, fn, label, cs, out, max_out, n_out: f(None, n_calls, first, n_frames, frames, fn,
                                                                                          label, cs, out, max_out, n_out)


def test_close_up_refusals_leave_the_outputs_alone(pkg):
    api = pkg.api
    a = audio_args(api)
    keep = _audio_outputs(a)
    good = _audio_good(a)
    f = _audio_call(api)
    p = lambda k: a[k].ctypes.data
    # everything gmr1_hip_tch3_frames_to_pcm_dev refuses (out in the place of pcm), then this entry's own
    bad = [dict(n_calls=-1), dict(n_frames=-1), dict(first=None), dict(frames=None), dict(out=None), dict(cs=None),
           dict(cs=p("cs") + 8), dict(cs=p("cs") + 4), dict(out=p("out") + 1),
           dict(fn=None), dict(label=None), dict(n_out=None), dict(out=p("out") + 2), dict(out=p("out") + 8), dict(max_out=-1)]
    for change in bad:
        assert f(**dict(good, **change)) == -EINVAL, change
        assert b"tch3_frames_to_audio" in api._fn("gmr1_hip_last_error")()
    assert _audio_outputs(a) == keep


def test_init_list_refusals_leave_the_states_alone(pkg):
    api = pkg.api
    a = audio_args(api)
    keep = a["cs"].tobytes()
    f = api._fn(NAMES[1])
    call, cs = a["call"].ctypes.data, a["cs"].ctypes.data
    for args in ((-1, call, cs, 0), (2, None, cs, 0), (2, call, None, 0), (2, call, cs + 8, 0), (2, call, cs, 2), (2, call, cs, -1)):
        assert f(None, *args) == -EINVAL, args
    assert a["cs"].tobytes() == keep


def _run_args(api, n=1000):
    return dict(iq=np.zeros(n, np.complex64), tch=np.zeros(n, np.complex64), offset=np.zeros(1, np.uint64),
                length=np.full(1, n, np.uint64), out=np.full(4 * 40, 0x11, np.uint8).view(api.RX_RECORD),
                audio=np.full(2 * 656, 0x5a, np.uint8).view(api.RX_AUDIO), n_rec=C.c_int(7), n_audio=C.c_int(7),
                status=np.full(1, 9, np.int32), chains=np.full(1, 9, np.int32))


def _run_voice(api, a, host, **change):
    p = lambda k: a[k].ctypes.data
    v = dict(audio=p("audio"), max_audio=2, n_audio=C.addressof(a["n_audio"]))
    v.update(change)
    tail = (p("offset"), p("length"), None, None, p("out"), a["out"].size, C.addressof(a["n_rec"]), p("status"), p("chains"),
            v["audio"], v["max_audio"], v["n_audio"])
    if host:
        return api._fn(NAMES[3])(1, 4, p("iq"), p("tch"), a["iq"].size, *tail)
    return api._fn(NAMES[2])(None, 1, 4, p("iq"), p("tch"), *tail)


def test_run_voice_refusals_leave_the_outputs_alone(pkg):
    api = pkg.api
    for host in (False, True):
        a = _run_args(api)
        keep = a["out"].tobytes() + a["audio"].tobytes() + a["status"].tobytes() + a["chains"].tobytes()
        for change in (dict(n_audio=None), dict(max_audio=-1), dict(audio=None)):
            assert _run_voice(api, a, host, **change) == -EINVAL, (host, change)
            assert b"rx_run_voice" in api._fn("gmr1_hip_last_error")()
        assert a["out"].tobytes() + a["audio"].tobytes() + a["status"].tobytes() + a["chains"].tobytes() == keep
        assert a["n_audio"].value == 0 and a["n_rec"].value == 0


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_the_calls_say_so(pkg):
    api = pkg.api
    a = audio_args(api)
    keep = _audio_outputs(a)
    f = _audio_call(api)
    assert f(**_audio_good(a)) == -ENODEV
    assert f(**dict(_audio_good(a), max_out=0, out=None)) == -ENODEV
    assert f(**dict(_audio_good(a), n_calls=-1)) == -EINVAL              # bad arguments come first
    assert api._fn(NAMES[1])(None, 2, a["call"].ctypes.data, a["cs"].ctypes.data, 0) == -ENODEV
    assert _audio_outputs(a) == keep
    for host in (False, True):
        r = _run_args(api)
        assert _run_voice(api, r, host) == -ENODEV
        assert _run_voice(api, r, host, max_audio=-1) == -EINVAL
    h = C.c_void_p()
    assert api._fn(NAMES[4])(1, 4, None, None, C.byref(h)) == -ENODEV and not h.value
    m = C.c_int(5)
    assert api._fn(NAMES[5])(None, 10, C.byref(m)) == -EINVAL
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.rx_run_voice(r["iq"], r["tch"], r["offset"], r["length"])
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.RxStream(1, voice=True)


# ---- tch3_audio.h and the carry rule on the host ----
def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "tch3_audio_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tch3audio"), "tch3_audio_host", [])


@pytest.fixture(scope="module")
def program_sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tch3audiosan"), "tch3_audio_host_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


SPANS = (0, 1, 63, 64, 65, 130)


def _cases():
    """(n_frames, first, cls, label, fn): random classes with OFF among them, calls of 0, 1, 63, 64, 65 and 130 frames in
    several orders, and first[] entries outside 0..n_frames, unordered ones among them"""
    rng = np.random.default_rng(656)
    out = [(0, [0], [], 0, 0), (0, [0, 0], [], 1, 2), (3, [0, 3], [0, 0, 0], 5, 6), (3, [0, 3], [4, 4, 4], 2 ** 40 - 1, 2 ** 32 - 1)]
    for it in range(60):
        spans = list(rng.permutation(SPANS)) if it % 2 else list(SPANS)
        first = np.concatenate([[0], np.cumsum(spans)])
        n = int(first[-1])
        cls = rng.integers(0, 6, n)
        if it % 5 == 0:
            cls[rng.random(n) < 0.5] = tc.OFF
        if it % 3 == 1:            # the ends leave 0..n_frames
            first[0], first[-1] = -int(rng.integers(1, 9)), n + int(rng.integers(1, 9))
        if it % 7 == 3:            # anything near the range, not ordered
            first = rng.integers(-5, n + 6, len(first))
        if it % 11 == 5:           # fewer frames than first[] says
            n = n // 2
            cls = cls[:n]
        out.append((n, [int(v) for v in first], [int(v) for v in cls], int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 32))))
    return out


def _check(exe):
    cases = _cases()
    text = "".join("%d %d %s %s %d %d\n" % (n, len(f) - 1, " ".join(map(str, f)), " ".join(map(str, c)), lab, fn)
                   for n, f, c, lab, fn in cases)
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    head = [int(x) for x in lines[0].split()]
    assert head[:256] == [int(c != tc.OFF) for c in range(256)]         # every class but OFF gives a block
    assert head[256:] == [656, 10, 16, 0, 0, -1]
    assert lines[1] == "carry ok"
    assert len(lines) - 3 == len(cases)
    seen_off = seen_clamped = 0
    for (n, first, cls, lab, fn), ln in zip(cases, lines[2:]):
        v = [int(x) for x in ln.split()]
        n_calls = len(first) - 1
        slot, base = vc.closeup(first, n, cls)
        assert v[:n] == list(slot), (n, first)
        assert v[n:n + n_calls + 1] == list(base), (n, first)
        c0 = cls[0] if n else 0
        assert v[n + n_calls + 1:] == [(lab & 0xffffff) | c0 << 24, fn, (lab >> 24) & 0xffff, 0]
        assert all(-1 <= s < max(n, 1) for s in slot)
        seen_off += any(c == tc.OFF for c in cls)
        seen_clamped += any(x < 0 or x > n for x in first)
        if first[0] == 0 and first[-1] == n and first == sorted(first):
            # a partition: the reporting frames take the slots 0, 1, 2, ... in frame order
            rep = [k for k in range(n) if cls[k] != tc.OFF]
            assert [slot[k] for k in rep] == list(range(len(rep))) and base[-1] == len(rep)
    assert seen_off and seen_clamped


def test_close_up_rule_equals_the_restatement(program):
    _check(program)


def test_close_up_rule_is_clean_under_asan_and_ubsan(program_sanitized):
    """The same check on the program built with -fsanitize=address,undefined (a stand-alone host program)."""
    _check(program_sanitized)
