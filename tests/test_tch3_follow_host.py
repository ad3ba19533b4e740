"""The batched TCH3 call follower (gmr1_hip_tch3_follow_batch*) without a GPU: it is declared, exported and mirrored with
the C layout, rx_tch3_init works on a caller-held state, bad arguments are refused, without a device the calls say so --
and the state machine the device runs (osmo-gmr_amd/csrc/tch3_follow.h), compiled for the host, reproduces the frame by
frame walk of tests/tch3_cases.py over the oracle's per-frame results."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tch3_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_tch3_state_assign", "gmr1_hip_tch3_follow_batch_dev", "gmr1_hip_tch3_follow_batch")
EINVAL, ENODEV = 22, 19


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:       # noqa: BLE001 - no torch, no device either
        return True


def _fields(txt, name):
    m = re.search(r"struct\s+%s\s*\{(.*?)\};" % name, txt, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for typ, names in re.findall(r"\b(int32_t|uint32_t|int8_t|uint8_t|float)\s+([^;]+);", body):
        out += [(typ, n.strip()) for n in names.split(",")]
    return out


def test_header_declares_the_structs_the_enum_and_the_calls():
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    assert _fields(txt, "gmr1_hip_tch3_state") == [
        ("int32_t", "active"), ("int32_t", "p"), ("int32_t", "ciph"), ("int32_t", "weak_cnt"), ("int32_t", "sync_id"),
        ("int32_t", "burst_cnt"), ("float", "energy_dkab"), ("float", "energy_burst"), ("uint32_t", "bi_fn[4]"),
        ("int8_t", "ebits[4 * 104]"), ("uint8_t", "kc[8]")]
    assert _fields(txt, "gmr1_hip_tch3_frame") == [
        ("uint8_t", "cls"), ("uint8_t", "type"), ("uint8_t", "len"), ("uint8_t", "ciph"), ("uint32_t", "fn"),
        ("int32_t", "conv"), ("float", "energy"), ("uint8_t", "l2[20]"), ("uint8_t", "pad[4]")]
    assert re.search(r"enum\s*\{\s*GMR1_HIP_TCH3_OFF\s*=\s*0\s*,\s*GMR1_HIP_TCH3_DKAB\s*,\s*GMR1_HIP_TCH3_DKAB_MISSING\s*,\s*"
                     r"GMR1_HIP_TCH3_FACCH\s*,\s*GMR1_HIP_TCH3_SPEECH\s*,\s*GMR1_HIP_TCH3_ERR\s*\}", txt)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert "gmr1_hip_tch3_follow_batch*" in txt.split("#ifndef GMR1_HIP_H")[0]        # the reference-interfaces list


def test_library_exports_the_symbols(pkg):
    lib = pkg.api.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pkg.api.SIGNATURES


def test_mirrors_have_the_c_layout(pkg, tmp_path):
    api = pkg.api
    assert api.TCH3_STATE.itemsize == C.sizeof(api.Tch3State) == 472
    assert api.TCH3_FRAME.itemsize == C.sizeof(api.Tch3Frame) == 40
    for cls, dt in ((api.Tch3State, api.TCH3_STATE), (api.Tch3Frame, api.TCH3_FRAME)):
        assert [n for n, _ in cls._fields_] == list(dt.names)
        for name, _ in cls._fields_:
            assert dt.fields[name][1] == getattr(cls, name).offset, name
    assert (api.TCH3_OFF, api.TCH3_DKAB, api.TCH3_DKAB_MISSING, api.TCH3_FACCH, api.TCH3_SPEECH, api.TCH3_ERR) == tuple(range(6))
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    st_f = [n for n, _ in api.Tch3State._fields_]
    fr_f = [n for n, _ in api.Tch3Frame._fields_]
    src = tmp_path / "tch3_size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmr1_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %d %d", sizeof(struct gmr1_hip_tch3_state), sizeof(struct gmr1_hip_tch3_frame), '
                   'GMR1_HIP_TCH3_OFF, GMR1_HIP_TCH3_ERR);\n'
                   + "".join('printf(" %%zu", offsetof(struct gmr1_hip_tch3_state, %s));\n' % n for n in st_f)
                   + "".join('printf(" %%zu", offsetof(struct gmr1_hip_tch3_frame, %s));\n' % n for n in fr_f)
                   + 'printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "tch3_size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert v[:4] == [472, 40, 0, 5]
    assert v[4:4 + len(st_f)] == [getattr(api.Tch3State, n).offset for n in st_f]
    assert v[4 + len(st_f):] == [getattr(api.Tch3Frame, n).offset for n in fr_f]


def test_state_assign_is_rx_tch3_init(pkg):
    """gmr1_rx.c:358-376: active, p, the two thresholds, weak_cnt, sync_id and the soft bits are set; ciph, burst_cnt, bi_fn
    (and the key) keep what they hold.  No device needed."""
    api = pkg.api
    st = np.zeros(2, api.TCH3_STATE)
    st["ciph"], st["burst_cnt"], st["weak_cnt"], st["sync_id"] = 1, 3, 7, 1
    st["bi_fn"] = [[11, 12, 13, 14], [21, 22, 23, 24]]
    st["ebits"] = 5
    st["kc"] = np.arange(16, dtype=np.uint8).reshape(2, 8)
    before = st.copy()
    assert api.tch3_state_assign(st, 33, 0.8, index=1) is st
    assert st[0] == before[0]
    s = st[1]
    assert (s["active"], s["p"], s["weak_cnt"], s["sync_id"]) == (1, 33, 0, 0)
    assert s["energy_burst"] == np.float32(0.8) * np.float32(0.75)
    assert s["energy_dkab"] == (np.float32(0.8) * np.float32(0.75)) / np.float32(8.0)
    assert not s["ebits"].any()
    assert (s["ciph"], s["burst_cnt"]) == (1, 3) and list(s["bi_fn"]) == [21, 22, 23, 24] and list(s["kc"]) == list(range(8, 16))
    assert api._fn(NAMES[0])(None, 0, 1.0) == -EINVAL


def _calls(api):
    """Both entries as f(n_calls, sps, in_len, iq, iq_len, first, n_frames, offset, fs, fn, state, out) -> return code, over host
    arrays (the _dev entry only looks at its arguments before it asks for the device)"""
    dev, host = api._fn(NAMES[1]), api._fn(NAMES[2])
    return [lambda n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out:
            dev(None, n_calls, sps, in_len, iq, first, n_frames, off, fs, fn, state, out),
            lambda n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out:
            host(n_calls, sps, in_len, iq, iq_len, first, n_frames, off, fs, fn, state, out)]


def test_bad_arguments_are_refused(pkg):
    api = pkg.api
    a = tc.call_args(api)
    a["state"]["active"] = 1
    keep_state, keep_out = a["state"].copy(), a["out"].copy()
    good, bad = tc.bad_argument_cases(a)
    for f in _calls(api):
        for change in bad:
            assert f(**dict(good, **change)) == -EINVAL, change
            assert b"tch3_follow" in api._fn("gmr1_hip_last_error")()
    # the host form knows how long iq is and sees the arrays: a window that leaves iq, a first[] that is not a partition
    host = _calls(api)[1]
    assert host(**dict(good, iq_len=1473)) == -EINVAL
    for first in ([1, 2], [0, 1], [0, 3]):
        a["first"][:] = first
        assert host(**good) == -EINVAL, first
    a["first"][:] = [0, 2]
    two = np.array([0, 2, 1], np.int32)
    assert host(**dict(good, n_calls=2, first=two.ctypes.data, n_frames=1)) == -EINVAL
    assert a["state"].tobytes() == keep_state.tobytes() and a["out"].tobytes() == keep_out.tobytes()


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_the_batch_calls_say_so(pkg):
    api = pkg.api
    a = tc.call_args(api)
    good, _ = tc.bad_argument_cases(a)
    for f in _calls(api):
        assert f(**good) == -ENODEV
        assert f(**dict(good, sps=0)) == -EINVAL           # bad arguments come first
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.tch3_follow(a["iq"], a["first"], a["off"], a["fs"], a["fn"], a["state"])


@pytest.fixture(scope="module")
def step_program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("tch3") / "tch3_follow_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "tch3_follow_host.cpp"), "-o", exe])
    return exe


def _bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("idx", [i for i, c in enumerate(tc.CASES) if c["sps"] == 4])
def test_step_function_walks_the_oracle_results(pkg, orc, step_program, idx):
    """tch3_follow.h on the CPU, fed the per-frame results the oracle computed: the classes, the decodes asked for, the
    flush points and the final state (but ciph, which the decodes decide) are those of the Python walk."""
    car = tc.carrier(pkg, idx)
    res = tc.frame_results(pkg, orc, idx)
    slots, margins, steps, end = tc.expected(pkg, orc, idx)
    assert min(margins) >= tc.MARGIN
    st0 = tc.initial_state(pkg, car)[0]
    lines = []
    for r in res:
        lines.append("%d %d %d %d %d %d %d %d" % (_bits(r["energy"]), r["dkab_rv"], r["det_rv"], r["btid"], r["facch_rv"],
                                                   r["facch_sid"], r["speech_rv"], r["fn"]))
        lines.append(" ".join(str(int(v)) for v in r["facch_eb"]))
    out = subprocess.run([step_program, str(int(st0["p"])), str(_bits(st0["energy_dkab"])), str(_bits(st0["energy_burst"]))],
                         input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
    got = [tuple(int(v) for v in ln.split()) for ln in out[:-1]]
    assert got == steps
    assert [g[0] for g in got] == [int(c) for c in slots["cls"]]
    tail = out[-1].split()
    assert tail[0] == "end"
    v = [int(x) for x in tail[1:]]
    e = end[0]
    assert v[:2] == [int(e["active"]), int(e["p"])] and v[3:6] == [int(e["weak_cnt"]), int(e["sync_id"]), int(e["burst_cnt"])]
    assert v[6:8] == [_bits(e["energy_dkab"]), _bits(e["energy_burst"])]       # same single-precision operations, in order
    assert v[8:12] == [int(x) for x in e["bi_fn"]]
    assert v[12:] == [int(x) for x in e["ebits"]]
    if idx == tc.ENDING:
        assert [g[0] for g in got].count(tc.DKAB_MISSING) == 10 and got[-1][0] == tc.OFF and v[0] == 0
