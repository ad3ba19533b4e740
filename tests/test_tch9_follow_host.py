"""The batched TCH9 call follower (gmr1_hip_tch9_follow*) without a GPU: its entries are declared, exported and mirrored
with the C layout, rx_tch9_init works on a caller-held state, bad arguments are refused before the device is asked for,
without a device the calls say so -- and the routing the device runs as a wave scan (osmo-gmr_amd/csrc/tch9_follow.h),
compiled for the host, gives the classes and de-interleaver sources of the frame by frame restatement in
tests/tch9_cases.py, cut anywhere."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tch9_cases as t9

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_tch9_state_assign", "gmr1_hip_tch9_state_assign_batch_dev", "gmr1_hip_tch9_follow_bits_batch_dev",
         "gmr1_hip_tch9_follow_bits_batch", "gmr1_hip_tch9_follow_batch_dev", "gmr1_hip_tch9_follow_batch")
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
    assert _fields(txt, "gmr1_hip_tch9_state") == [
        ("int32_t", "active"), ("int32_t", "n_held"), ("uint8_t", "kc[8]"), ("int8_t", "held[2 * 662]")]
    assert _fields(txt, "gmr1_hip_tch9_frame") == [
        ("uint8_t", "cls"), ("uint8_t", "type"), ("uint8_t", "len"), ("uint8_t", "crc"), ("uint32_t", "fn"),
        ("int32_t", "conv"), ("uint8_t", "l2[64]"), ("uint8_t", "pad[4]")]
    assert re.search(r"enum\s*\{\s*GMR1_HIP_TCH9_OFF\s*=\s*0\s*,\s*GMR1_HIP_TCH9_FACCH9\s*,\s*GMR1_HIP_TCH9_TCH9\s*,\s*"
                     r"GMR1_HIP_TCH9_ERR\s*\}", txt)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert "gmr1_hip_tch9_follow*_batch*" in txt.split("#ifndef GMR1_HIP_H")[0]       # the reference-interfaces list


def test_library_exports_the_symbols(pkg):
    lib = pkg.api.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pkg.api.SIGNATURES
    for name in ("tch9_state_assign", "tch9_state_assign_batch_dev", "tch9_follow_bits", "tch9_follow_bits_dev", "tch9_follow",
                 "tch9_follow_dev"):
        assert callable(getattr(pkg.api, name)), name


def test_mirrors_have_the_c_layout(pkg, tmp_path):
    api = pkg.api
    assert api.TCH9_STATE.itemsize == 1340 and api.TCH9_FRAME.itemsize == 80
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    for struct, dt in (("gmr1_hip_tch9_state", api.TCH9_STATE), ("gmr1_hip_tch9_frame", api.TCH9_FRAME)):
        assert [n.split("[")[0] for _, n in _fields(txt, struct)] == list(dt.names)
    assert (api.TCH9_OFF, api.TCH9_FACCH9, api.TCH9_TCH9, api.TCH9_ERR) == tuple(range(4))
    assert (t9.OFF, t9.FACCH9, t9.TCH9, t9.ERR) == tuple(range(4))
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    st_f, fr_f = list(api.TCH9_STATE.names), list(api.TCH9_FRAME.names)
    src = tmp_path / "tch9_size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmr1_hip.h"\n'
                   '_Static_assert(sizeof(struct gmr1_hip_tch9_state) == 1340, "state");\n'
                   '_Static_assert(sizeof(struct gmr1_hip_tch9_frame) == 80, "frame");\nint main(void) {\n'
                   'printf("%zu %zu %d %d", sizeof(struct gmr1_hip_tch9_state), sizeof(struct gmr1_hip_tch9_frame), '
                   'GMR1_HIP_TCH9_OFF, GMR1_HIP_TCH9_ERR);\n'
                   + "".join('printf(" %%zu", offsetof(struct gmr1_hip_tch9_state, %s));\n' % n for n in st_f)
                   + "".join('printf(" %%zu", offsetof(struct gmr1_hip_tch9_frame, %s));\n' % n for n in fr_f)
                   + 'printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "tch9_size")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert v[:4] == [1340, 80, 0, 3]
    assert v[4:4 + len(st_f)] == [api.TCH9_STATE.fields[n][1] for n in st_f]
    assert v[4 + len(st_f):] == [api.TCH9_FRAME.fields[n][1] for n in fr_f]


def test_state_assign_is_rx_tch9_init(pkg):
    """gmr1_rx.c:263-274: the call is active and its interleaver fresh; the key keeps what it holds.  No device needed."""
    api = pkg.api
    st = np.zeros(2, api.TCH9_STATE)
    st["n_held"] = 2
    st["held"] = 5
    st["kc"] = np.arange(16, dtype=np.uint8).reshape(2, 8)
    before = st.copy()
    assert api.tch9_state_assign(st, index=1) is st
    assert st[0] == before[0]
    s = st[1]
    assert (s["active"], s["n_held"]) == (1, 0) and not s["held"].any() and list(s["kc"]) == list(range(8, 16))
    assert api._fn(NAMES[0])(None) == -EINVAL
    dev = api._fn(NAMES[1])
    call = np.zeros(1, np.int32)
    assert dev(None, -1, call.ctypes.data, st.ctypes.data) == -EINVAL
    assert dev(None, 1, None, st.ctypes.data) == -EINVAL and dev(None, 1, call.ctypes.data, None) == -EINVAL


def _bits_calls(api):
    dev, host = api._fn(NAMES[2]), api._fn(NAMES[3])
    return [lambda n_calls, mode, first, n_frames, ebits, sid, rv, fn, state, out:
            dev(None, n_calls, mode, first, n_frames, ebits, sid, rv, fn, state, out),
            lambda n_calls, mode, first, n_frames, ebits, sid, rv, fn, state, out:
            host(n_calls, mode, first, n_frames, ebits, sid, rv, fn, state, out)]


def _samples_calls(api):
    dev, host = api._fn(NAMES[4]), api._fn(NAMES[5])
    return [lambda n_calls, sps, in_len, mode, iq, iq_len, first, n_frames, off, fs, fn, state, out:
            dev(None, n_calls, sps, in_len, mode, iq, first, n_frames, off, fs, fn, state, out),
            lambda n_calls, sps, in_len, mode, iq, iq_len, first, n_frames, off, fs, fn, state, out:
            host(n_calls, sps, in_len, mode, iq, iq_len, first, n_frames, off, fs, fn, state, out)]


def test_bad_arguments_are_refused(pkg):
    api = pkg.api
    for args, cases, calls in ((t9.bits_args, t9.bits_bad_cases, _bits_calls), (t9.samples_args, t9.samples_bad_cases, _samples_calls)):
        a = args(api)
        a["state"]["active"] = 1
        keep_state, keep_out = a["state"].copy(), a["out"].copy()
        good, bad = cases(a)
        for f in calls(api):
            for change in bad:
                assert f(**dict(good, **change)) == -EINVAL, change
                assert b"tch9_follow" in api._fn("gmr1_hip_last_error")()
        # the host forms see the arrays: a first[] that is not a partition (and a window that leaves iq)
        host = calls(api)[1]
        for first in ([1, 2], [0, 1], [0, 3]):
            a["first"][:] = first
            assert host(**good) == -EINVAL, first
        a["first"][:] = [0, 2]
        two = np.array([0, 2, 1], np.int32)
        assert host(**dict(good, n_calls=2, first=two.ctypes.data, n_frames=1)) == -EINVAL
        if "iq_len" in good:
            assert host(**dict(good, iq_len=2409)) == -EINVAL
        assert a["state"].tobytes() == keep_state.tobytes() and a["out"].tobytes() == keep_out.tobytes()


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_the_batch_calls_say_so(pkg):
    api = pkg.api
    a = t9.bits_args(api)
    good, _ = t9.bits_bad_cases(a)
    for f in _bits_calls(api):
        assert f(**good) == -ENODEV
        assert f(**dict(good, rv=None)) == -ENODEV            # rv may be left out
        assert f(**dict(good, mode=3)) == -EINVAL             # bad arguments come first
    b = t9.samples_args(api)
    good, _ = t9.samples_bad_cases(b)
    for f in _samples_calls(api):
        assert f(**good) == -ENODEV
        assert f(**dict(good, sps=0)) == -EINVAL
    call = np.zeros(1, np.int32)
    assert api._fn(NAMES[1])(None, 1, call.ctypes.data, a["state"].ctypes.data) == -ENODEV
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.tch9_follow_bits(a["first"], a["ebits"], a["sid"], a["fn"], a["state"])
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.tch9_follow(b["iq"], b["first"], b["off"], b["fs"], b["fn"], b["state"])


# ---- tch9_follow.h against the frame by frame restatement ----
def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "tch9_follow_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tch9"), "tch9_follow_host", [])


@pytest.fixture(scope="module")
def plan_program_sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tch9san"), "tch9_follow_host_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _plan(exe, jobs):
    """jobs: (active, n_held, base, rv, sync_id) -> per job ([(cls, need, s1, s2)], (s1, s2), n_held)"""
    text = "".join("%d %d %d %d %s\n" % (a, nh, base, len(rv), " ".join("%d %d" % p for p in zip(rv, sid)))
                   for a, nh, base, rv, sid in jobs)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(jobs)
    res = []
    for ln in out:
        v = [int(x) for x in ln.split()]
        n = (len(v) - 3) // 4
        res.append(([tuple(v[4 * k:4 * k + 4]) for k in range(n)], (v[-3], v[-2]), v[-1]))
    return res


def _sequences():
    rng = np.random.default_rng(99)
    seqs = []
    for n in [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200] + [int(x) for x in rng.integers(0, 201, 12)]:
        p_tch = rng.choice([0.05, 0.5, 0.95])
        rv = np.where(rng.random(n) < 0.15, rng.choice([-1, -5, 1], n), 0)
        sid = np.where(rng.random(n) < p_tch, rng.choice([1, 2, 3], n), 0)
        seqs.append(([int(x) for x in rv], [int(x) for x in sid]))
    return seqs


def _check_whole(exe):
    jobs, want = [], []
    for rv, sid in _sequences():
        for nh in (0, 1, 2):
            for active, base in ((1, 0), (1, 37), (0, 0)):
                jobs.append((active, nh, base, rv, sid))
                want.append(t9.route(active, nh, rv, sid, base))
    got = _plan(exe, jobs)
    for job, (frames, carry, nh), (w_frames, w_carry) in zip(jobs, got, want):
        assert frames == w_frames, job[:3]
        assert carry == w_carry and nh == sum(s != t9.SRC_ZEROS for s in w_carry), job[:3]


def test_scan_equals_the_frame_by_frame_walk(plan_program):
    """Random (rv, sync_id) sequences of 0..200 frames under all three n_held, from frame 0 and from another base, active or
    not: classes, decodes asked for, both sources of every frame and the carry behind the last one."""
    _check_whole(plan_program)


def _absolute(src, carry_in):
    """a piece's held slots are what the cut passed on: the uncut sequence's sources at the cut"""
    return carry_in[0] if src == t9.SRC_HELD0 else carry_in[1] if src == t9.SRC_HELD1 else src


def _check_cuts(exe):
    rng = np.random.default_rng(5)
    for n, nh0 in ((9, 0), (70, 1), (131, 2)):
        rv = [int(x) for x in np.where(rng.random(n) < 0.2, -1, 0)]
        sid = [int(x) for x in (rng.random(n) < 0.6)]
        whole, w_carry = t9.route(1, nh0, rv, sid)
        # piece 1 of every cut, then piece 2 seeded with piece 1's n_held
        ones = _plan(exe, [(1, nh0, 0, rv[:p], sid[:p]) for p in range(n + 1)])
        twos = _plan(exe, [(1, ones[p][2], p, rv[p:], sid[p:]) for p in range(n + 1)])
        for p in range(n + 1):
            f1, c1, nh1 = ones[p]
            f2, c2, _ = twos[p]
            assert f1 == whole[:p], (n, p)
            # what piece 2 finds in the state is piece 1's carry, in absolute terms of the uncut sequence
            seen = [(c, nd, _absolute(s1, c1), _absolute(s2, c1)) for c, nd, s1, s2 in f2]
            assert seen == whole[p:], (n, p)
            assert (_absolute(c2[0], c1), _absolute(c2[1], c1)) == w_carry, (n, p)
            # a frame index never turns into zeros: the state holds as many bursts as the carry names
            assert nh1 == sum(s != t9.SRC_ZEROS for s in c1)


def test_a_cut_anywhere_keeps_every_source(plan_program):
    """Cutting a sequence at every position: every frame of both pieces has the uncut sequence's sources -- a frame index
    of the first piece has become a held slot of the second, never zeros."""
    _check_cuts(plan_program)


def test_the_routing_is_clean_under_asan_and_ubsan(plan_program_sanitized):
    """The same two checks on the program built with -fsanitize=address,undefined (a stand-alone host program)."""
    _check_whole(plan_program_sanitized)
    _check_cuts(plan_program_sanitized)
