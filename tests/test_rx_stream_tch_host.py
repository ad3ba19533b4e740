"""The streaming receive loop's TCH3 follow-up without a GPU: the four new entries are declared and exported, refuse bad
arguments and say -ENODEV without a device; the arithmetic that makes a push's traffic windows the one-shot call's
(osmo-gmr_amd/csrc/rx_stream.h, compiled for the host) holds for sps 1..16; and the assign function the host entry and
k_tch3f_assign share (tch3_follow.h) is the oracle's rx_tch3_init."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_rx_stream_create_tch", "gmr1_hip_rx_stream_push_tch_dev", "gmr1_hip_rx_stream_push_tch",
         "gmr1_hip_tch3_state_assign_batch_dev")
EINVAL, ENODEV = 22, 19


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
    assert "TCH3 / TCH9 follow-ups are not performed" not in txt


def test_bad_arguments_are_refused_before_the_device_is_asked(pkg):
    """what needs no handle to be judged: -EINVAL with or without a device"""
    api = pkg.api
    h = C.c_void_p(5)
    create, assign = api._fn(NAMES[0]), api._fn(NAMES[3])
    for n_arfcn, sps in ((0, 4), (65536, 4), (2, 0), (2, 17)):
        assert create(n_arfcn, sps, None, None, C.byref(h)) == -EINVAL
        assert h.value is None
    assert create(2, 4, None, None, None) == -EINVAL
    a = np.zeros(4, np.int32)
    e = np.zeros(4, np.float32)
    st = np.zeros(4, api.TCH3_STATE)
    p = lambda v: v.ctypes.data
    assert assign(None, -1, p(a), p(a), p(e), p(st)) == -EINVAL
    for bad in range(4):
        args = [p(a), p(a), p(e), p(st)]
        args[bad] = None
        assert assign(None, 4, *args) == -EINVAL
    assert b"tch3_state_assign_batch" in api._fn("gmr1_hip_last_error")()
    assert not st.view(np.uint8).any()


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_the_new_entries_say_so(pkg):
    api = pkg.api
    h, m = C.c_void_p(), C.c_int()
    a = np.zeros(4, np.int32)
    e = np.zeros(4, np.float32)
    st = np.zeros(4, api.TCH3_STATE)
    assert api._fn(NAMES[0])(4, 4, None, None, C.byref(h)) == -ENODEV
    assert api._fn(NAMES[1])(None, None, None, None, 0, 0, 1, None, 0, C.byref(m)) == -ENODEV
    assert api._fn(NAMES[2])(None, None, None, 0, 0, 1, None, 0, C.byref(m)) == -ENODEV
    assert api._fn(NAMES[3])(None, 4, a.ctypes.data, a.ctypes.data, e.ctypes.data, st.ctypes.data) == -ENODEV
    assert not st.view(np.uint8).any()
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.RxStream(4, sps=4, tch=True)
    with pytest.raises(ValueError):
        api.RxStream(4, sps=4, kc=np.zeros((4, 8), np.uint8))


def test_traffic_windows_fit_what_the_walk_admitted(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "rx_stream_tch_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "rx_stream_tch_host.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


def test_shared_assign_is_the_oracles_rx_tch3_init(pkg, orc, tmp_path):
    """gmr1_hip_tch3_state_assign -- tch3_follow_assign of tch3_follow.h, which k_tch3f_assign runs on the device -- against
    rx_tch3_init of oracle/orc_rx.c on random states: every field the reference writes is written alike, and ciph,
    burst_cnt, bi_fn and the key keep their values."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    api = pkg.api
    odir = os.path.dirname(orc.LIB_PATH)
    so = str(tmp_path / "libtch3_init_oracle.so")
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-shared", "-fPIC",
                           "-I" + odir, os.path.join(ROOT, "tests", "c", "tch3_init_oracle.c"), "-o", so,
                           "-L" + odir, "-lorc", "-Wl,-rpath," + odir, "-lm"])
    f = C.CDLL(so).tch3_init_oracle
    f.restype = C.c_int
    f.argtypes = (C.c_void_p, C.c_int, C.c_int, C.c_float)
    rng = np.random.default_rng(12)
    n = 200
    state = np.frombuffer(rng.integers(0, 256, n * api.TCH3_STATE.itemsize, dtype=np.uint8).tobytes(), api.TCH3_STATE).copy()
    state["energy_dkab"] = rng.random(n, dtype=np.float32)
    state["energy_burst"] = rng.random(n, dtype=np.float32)
    flat = np.dtype([(k, api.TCH3_STATE.fields[k][0]) for k in api.TCH3_STATE.names if k != "kc"])
    assert flat.itemsize == api.TCH3_STATE.fields["kc"][1] == 464
    for k in range(n):
        tn, p = int(rng.integers(0, 32)), int(rng.integers(0, 64))
        en = float(np.float32(rng.random() * 10.0 ** rng.integers(-3, 4)))
        before = state[k].copy()
        want = np.zeros(1, flat)
        for name in flat.names:
            want[name][0] = before[name]
        assert f(want.ctypes.data, tn, p, en) == tn
        api.tch3_state_assign(state, p, en, index=k)
        got = state[k]
        for name in flat.names:
            assert np.array_equal(got[name], want[name][0]), (k, name)
        assert got.tobytes()[:464] == want.tobytes()
        for name in ("ciph", "burst_cnt", "bi_fn", "kc"):
            assert np.array_equal(got[name], before[name]), (k, name)
        assert got["active"] == 1 and got["p"] == p and not got["ebits"].any()
