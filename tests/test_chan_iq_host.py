"""Integer IQ captures into the channelizer and the direct mode (gmr1_hip_*_iq*), what can be said without a GPU: the entries
are declared, exported and mirrored with the header's arity; gmr1_hip_iq_sample_bytes is host arithmetic; and THE load rule
every kernel reads a capture through (osmo-gmr_amd/csrc/iq_format.h, compiled for the host by tests/c/iq_format_host.cpp)
turns every int16 and every int8 value into exactly np.float32(v) * 2^-15 / 2^-7, read out of a buffer whose base lies one
sample into its allocation.  Once plain, once under the address and undefined-behaviour sanitizers (a stand-alone program:
nothing is preloaded)."""
import os
import re

import numpy as np
import pytest

import test_chan_select_host as host

ROOT = host.ROOT
# name -> arguments in the header
NAMES = {
    "gmr1_hip_iq_sample_bytes": 1,
    "gmr1_hip_channelize_iq_dev": 12,
    "gmr1_hip_channelize_iq": 11,
    "gmr1_hip_channelize_planar_iq_dev": 13,
    "gmr1_hip_ddc_iq_dev": 11,
    "gmr1_hip_ddc_iq": 10,
    "gmr1_hip_channelize_stream_create_iq": 7,
    "gmr1_hip_ddc_stream_create_iq": 6,
    "gmr1_hip_chan_stream_push_iq_dev": 7,
    "gmr1_hip_chan_stream_push_iq": 6,
}
EINVAL, ENODEV = 22, 19


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:       # noqa: BLE001 - no torch, no device either
        return True


def test_header_declares_the_enum_and_the_calls():
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    assert re.search(r"enum\s*\{\s*GMR1_HIP_IQ_F32\s*=\s*0\s*,\s*GMR1_HIP_IQ_S16\s*=\s*1\s*,\s*GMR1_HIP_IQ_S8\s*=\s*2\s*\}", txt)
    for name, n_args in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        if name != "gmr1_hip_iq_sample_bytes" and "create" not in name:
            assert "const void *wide" in m.group(1), name          # no float in the type: the format says what it is
        if "push" not in name:
            assert "int fmt" in m.group(1), name


def test_library_exports_and_api_mirrors_them(pkg):
    api = pkg.api
    lib = api.load()
    for name, n_args in NAMES.items():
        assert hasattr(lib, name), name
        assert len(api.SIGNATURES[name]) == n_args + 1, name       # (result, arguments ...)
    # an _iq prototype is its float neighbour's with the format put in (creates, one-shot) or as it is (pushes)
    for name in NAMES:
        twin = name.replace("_iq", "")
        if twin in api.SIGNATURES and "push" in name:
            assert api.SIGNATURES[name] == api.SIGNATURES[twin], name
        elif twin in api.SIGNATURES:
            sig, tw = list(api.SIGNATURES[name]), list(api.SIGNATURES[twin])
            k = 4 if name.endswith("_dev") else 3                  # (result, [stream,] samp_rate, sps, fmt, ...
            assert sig[:k] + sig[k + 1:] == tw and sig[k] is api.SIGNATURES["gmr1_hip_iq_sample_bytes"][1], name
    for name in ("channelize_iq", "ddc_iq", "channelize_iq_dev", "ddc_iq_dev", "channelize_planar_iq_dev", "iq_sample_bytes"):
        assert callable(getattr(api, name)), name
    assert (api.IQ_F32, api.IQ_S16, api.IQ_S8) == (0, 1, 2)


def test_sample_bytes_is_host_arithmetic(pkg):
    lib = pkg.api.load()
    assert [lib.gmr1_hip_iq_sample_bytes(f) for f in (0, 1, 2)] == [8, 4, 2]
    assert lib.gmr1_hip_iq_sample_bytes(-1) == -EINVAL and lib.gmr1_hip_iq_sample_bytes(3) == -EINVAL
    assert [pkg.api.iq_sample_bytes(f) for f in (pkg.api.IQ_F32, pkg.api.IQ_S16, pkg.api.IQ_S8)] == [8, 4, 2]
    with pytest.raises(pkg.api.Gmr1HipError, match="-22"):
        pkg.api.iq_sample_bytes(3)


def test_python_takes_the_format_from_the_dtype(pkg):
    api = pkg.api
    for dt, fmt in ((np.int16, api.IQ_S16), (np.int8, api.IQ_S8)):
        a, f, n = api._iq(np.zeros((7, 2), dt))
        assert (f, n, a.dtype) == (fmt, 7, dt)
        with pytest.raises(ValueError):
            api._iq(np.zeros(14, dt))                              # flat integers: which is I, which is Q?
        with pytest.raises(TypeError):
            api._iq(np.zeros((7, 2), dt), api.IQ_F32)              # a float handle is not pushed integers
    a, f, n = api._iq(np.zeros(7, np.complex64))
    assert (f, n) == (api.IQ_F32, 7)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the device tests cover the calls")
def test_without_a_device_the_calls_say_so(pkg):
    api = pkg.api
    x = np.zeros((64, 2), np.int16)
    with pytest.raises(api.Gmr1HipError, match="-%d" % ENODEV):
        api.channelize_iq(x, 2.0e6, [5])
    with pytest.raises(api.Gmr1HipError, match="-%d" % ENODEV):
        api.ddc_iq(x, 2.0e6, [0.0])
    with pytest.raises(api.Gmr1HipError, match="-%d" % ENODEV):
        api.ChanStream(2.0e6, [5], fmt=api.IQ_S16)
    with pytest.raises(api.Gmr1HipError, match="-%d" % ENODEV):
        api.ChanStream.direct(2.0e6, [0.0], fmt=api.IQ_S8)


@pytest.fixture(scope="module", params=([], host.SAN), ids=("plain", "asan_ubsan"))
def rule(request, tmp_path_factory):
    exe = host._build(tmp_path_factory.mktemp("iq_format"), request.param, "iq_format_host")
    out = {}
    for ln in host._run(exe, [], "").splitlines():
        w = ln.split()
        out[w[0]] = w[2:]
        assert len(w) - 2 == int(w[1]), w[0]
    return out


def _f32(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def test_load_rule_bytes_and_scale(rule):
    assert [int(v) for v in rule["bytes"]] == [8, 4, 2, -1, -1]
    assert np.array_equal(_f32(rule["scale"]), np.array([1.0, 2.0 ** -15, 2.0 ** -7], np.float32))


@pytest.mark.parametrize("name,dtype,k", [("s16", np.int16, 15), ("s8", np.int8, 7)])
def test_load_rule_on_every_value(rule, name, dtype, k):
    """bit for bit (the words are compared, so a -0.0 for 0 or a denormal flushed would show)"""
    info = np.iinfo(dtype)
    v = np.arange(info.min, info.max + 1, dtype=np.int64)
    want_i = v.astype(dtype).astype(np.float32) * np.float32(2.0 ** -k)
    want_q = (~v).astype(dtype).astype(np.float32) * np.float32(2.0 ** -k)
    got_i, got_q = _f32(rule[name + "_i"]), _f32(rule[name + "_q"])
    assert got_i.size == v.size and got_q.size == v.size
    assert np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32))
    assert np.array_equal(got_q.view(np.uint32), want_q.view(np.uint32))
    assert got_i[0] == -1.0 and got_i[-1] == np.float32(info.max) / np.float32(-float(info.min))


def test_load_rule_float_is_a_plain_read(rule):
    want = np.array([0.25, -1.5, 3.0e-39, -0.0], np.float32)
    assert np.array_equal(_f32(rule["f32"]).view(np.uint32), want.view(np.uint32))
