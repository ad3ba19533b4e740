"""The streaming receive loop's TCH9 follow-up without a GPU: the new entries are declared, exported and bound, refuse bad
arguments before the device is asked for and say -ENODEV without one; and the integer rules that make a push's NT9 frames
the one-shot call's (tch9_plan_push of osmo-gmr_amd/csrc/rx_follow.h, cut into pushes, against the reference's frame loop
restated in tests/c/rx_tch9_ref.h: the frames it maps, the command in force and every TCH9 burst's interleaver position;
the window fit and the big-record bound of rx_stream.h; tests/c/rx_stream_full_host.cpp, compiled for the host) hold -- once plain,
once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_rx_stream_create_full", "gmr1_hip_rx_stream_max_big", "gmr1_hip_rx_stream_push_full_dev",
         "gmr1_hip_rx_stream_push_full", "gmr1_hip_tch9_frames_to_records_dev")
EINVAL, ENODEV = 22, 19
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:       # noqa: BLE001 - no torch, no device either
        return True


def test_header_and_library_have_the_new_entries(pkg):
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    lib = pkg.api.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in pkg.api.SIGNATURES
    assert "follow-ups are not performed by either" not in txt
    # the header says where the one-shot call and the full handle part at sps 12
    assert re.search(r"_create_full refuses sps > 11", txt)


def _frames_args(api, n_calls=2, n_frames=4):
    first = np.zeros(n_calls + 1, np.int32)
    frames = np.zeros(n_frames, api.TCH9_FRAME)
    label = np.zeros(n_calls, np.uint32)
    out = np.zeros(n_frames + 1, api.RX_BIG_RECORD)      # (numpy's memory is on a 16-byte boundary)
    n_out = np.full(1, 7, np.int32)
    return first, frames, label, out, n_out


def test_bad_arguments_are_refused_before_the_device_is_asked(pkg):
    """what needs no handle to be judged: -EINVAL with or without a device"""
    api = pkg.api
    p = lambda v: v.ctypes.data
    h = C.c_void_p(5)
    create, max_big, push_dev, push, to_rec = (api._fn(n) for n in NAMES)
    # sps 12 on: the NT9 window is above GMR1_HIP_MAX_IN_LEN
    for n_arfcn, sps in ((0, 4), (65536, 4), (2, 0), (2, 17), (2, 12), (2, 16)):
        h.value = 5
        assert create(n_arfcn, sps, None, None, C.byref(h)) == -EINVAL, (n_arfcn, sps)
        assert h.value is None
    assert b"NT9 window" in api._fn("gmr1_hip_last_error")()
    assert create(2, 4, None, None, None) == -EINVAL
    m = C.c_int(7)
    assert max_big(None, 100, C.byref(m)) == -EINVAL and m.value == 7
    assert max_big(C.c_void_p(5), 100, None) == -EINVAL
    n_rec, n_big = C.c_int(7), C.c_int(7)
    assert push(None, None, None, None, 0, 0, 1, None, 0, C.byref(n_rec), None, 0, C.byref(n_big)) == -EINVAL
    assert n_rec.value == 0 and n_big.value == 0
    assert push_dev(None, None, None, None, None, 0, 0, 1, None, 0, C.byref(n_rec), None, 0, C.byref(n_big)) == -EINVAL
    fake = C.c_void_p(5)        # never dereferenced: the counts are judged first
    for f, head in ((push, (fake,)), (push_dev, (None, fake))):
        assert f(*head, None, None, None, 0, 0, 1, None, 0, None, None, 0, C.byref(n_big)) == -EINVAL
        assert f(*head, None, None, None, 0, 0, 1, None, 0, C.byref(n_rec), None, 0, None) == -EINVAL
        assert f(*head, None, None, None, 0, 0, 1, None, -1, C.byref(n_rec), None, 0, C.byref(n_big)) == -EINVAL
        assert f(*head, None, None, None, 0, 0, 1, None, 0, C.byref(n_rec), None, -1, C.byref(n_big)) == -EINVAL
    # the frames-to-records entry
    first, frames, label, out, n_out = _frames_args(api)
    good = [None, 2, p(first), 4, p(frames), p(label), p(out), 4, p(n_out)]
    for at, bad in ((1, -1), (3, -1), (7, -1), (2, None), (4, None), (5, None), (8, None), (6, None), (6, p(out) + 8)):
        args = list(good)
        args[at] = bad
        assert to_rec(*args) == -EINVAL, (at, bad)
    assert b"tch9_frames_to_records" in api._fn("gmr1_hip_last_error")()
    assert n_out[0] == 7 and not out.view(np.uint8).any()


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_the_new_entries_say_so(pkg):
    api = pkg.api
    p = lambda v: v.ctypes.data
    h = C.c_void_p()
    fake = C.c_void_p(5)        # never dereferenced: there is no device to make a handle on
    m, n_rec, n_big = C.c_int(), C.c_int(), C.c_int()
    create, max_big, push_dev, push, to_rec = (api._fn(n) for n in NAMES)
    assert create(4, 4, None, None, C.byref(h)) == -ENODEV and h.value is None
    assert create(4, 11, None, None, C.byref(h)) == -ENODEV
    assert max_big(fake, 100, C.byref(m)) == -ENODEV
    assert push(fake, None, None, None, 0, 0, 1, None, 0, C.byref(n_rec), None, 0, C.byref(n_big)) == -ENODEV
    assert push_dev(None, fake, None, None, None, 0, 0, 1, None, 0, C.byref(n_rec), None, 0, C.byref(n_big)) == -ENODEV
    first, frames, label, out, n_out = _frames_args(api)
    assert to_rec(None, 2, p(first), 4, p(frames), p(label), p(out), 4, p(n_out)) == -ENODEV
    assert to_rec(None, 0, p(first), 0, p(frames), p(label), None, 0, p(n_out)) == -ENODEV
    assert n_out[0] == 7 and not out.view(np.uint8).any()
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.RxStream(4, sps=4, full=True)
    with pytest.raises(api.Gmr1HipError, match="-22"):
        api.RxStream(4, sps=12, full=True)


@pytest.mark.parametrize("extra", ([], SAN), ids=("plain", "asan_ubsan"))
def test_pushes_plan_the_one_shot_frames_and_their_windows_fit(tmp_path, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "rx_stream_full_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra +
                          ["-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "rx_stream_full_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


def test_ass_cmd_takes_a_list_of_commands(pkg):
    """synth_tch3_carrier: a message at frame >= k names the timeslot of the last list entry it has reached; a single tuple
    is what it was"""
    from importlib import import_module
    synth = import_module(pkg.__name__ + ".synth")
    fs, ff = pkg.api.burst_format("nt3_speech"), pkg.api.burst_format("nt3_facch")
    n = int(3.0 * 23400 * 4)

    def sent(ass_cmd):
        rng = np.random.default_rng(5)
        x, s = synth.synth_tch3_carrier(fs, ff, n, 4, rng, t0=100, fn0=8, k_start=2, tn=3, p=7, mix=(0.1, 0.1, 0.8), ass_cmd=ass_cmd)
        return x, [(m["k"], bytes(m["l2"])) for m in s if m["type"] == "facch3"]

    def named(l2):
        return ((l2[5] & 3) << 3) | (l2[6] >> 5) if l2[3] == 0x06 and l2[4] == 0x2e else None

    x1, one = sent((20, 9))
    x2, as_list = sent([(20, 9)])
    assert one == as_list and np.array_equal(x1, x2)
    _, two = sent([(40, 14), (20, 5)])
    got = [(k, named(l2)) for k, l2 in two]
    assert [t for k, t in got if k < 20] and all(t is None for k, t in got if k < 20)
    assert {t for k, t in got if 20 <= k < 40} == {5} and {t for k, t in got if k >= 40} == {14}
