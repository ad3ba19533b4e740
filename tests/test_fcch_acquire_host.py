"""The batched FCCH acquisition entry (gmr1_hip_fcch_acquire_batch*) without a GPU: it is declared, exported and mirrored
with the C layout, refuses bad arguments, and without a device says so instead of computing anything."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmr1_hip_fcch_acquire_batch_dev", "gmr1_hip_fcch_acquire_batch")
EINVAL, ENODEV = 22, 19


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:       # noqa: BLE001 - no torch, no device either
        return True


def test_header_declares_the_struct_and_both_calls():
    txt = open(os.path.join(ROOT, "include", "gmr1_hip.h")).read()
    assert re.search(r"#define\s+GMR1_HIP_ACQ_MAX_CHAINS\s+16\b", txt)
    m = re.search(r"struct\s+gmr1_hip_fcch_acq\s*\{(.*?)\};", txt, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+)(\[GMR1_HIP_ACQ_MAX_CHAINS\])?\s*;", body)
    assert [(t, n, bool(a)) for t, n, a in fields] == [
        ("int32_t", "status", False), ("int32_t", "n_chains", False), ("int32_t", "align", False),
        ("int32_t", "base_align", False), ("float", "freq_err", False), ("int32_t", "n_cand", False),
        ("int32_t", "chain_align", True), ("float", "chain_freq_err", True), ("float", "chain_snr", True)]
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name


def test_library_exports_both_symbols(pkg):
    lib = pkg.api.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pkg.api.SIGNATURES


def test_mirrors_have_the_c_layout(pkg, tmp_path):
    api = pkg.api
    assert api.FCCH_ACQ.itemsize == C.sizeof(api.FcchAcq) == 24 + 3 * 4 * api.ACQ_MAX_CHAINS
    for name, _ in api.FcchAcq._fields_:
        assert api.FCCH_ACQ.fields[name][1] == getattr(api.FcchAcq, name).offset, name
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "acq_size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmr1_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d\\n", sizeof(struct gmr1_hip_fcch_acq), '
                   'offsetof(struct gmr1_hip_fcch_acq, chain_align), offsetof(struct gmr1_hip_fcch_acq, chain_snr), '
                   'GMR1_HIP_ACQ_MAX_CHAINS); return 0; }\n')
    exe = str(tmp_path / "acq_size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, o_align, o_snr, slots = (int(v) for v in subprocess.check_output([exe], text=True).split())
    assert size == C.sizeof(api.FcchAcq) and slots == api.ACQ_MAX_CHAINS
    assert o_align == api.FcchAcq.chain_align.offset and o_snr == api.FcchAcq.chain_snr.offset


def _calls(api):
    """Both entries as f(fcch_type, n, sps, iq, offset, length, start, out) -> return code, over host arrays (the _dev entry
    only looks at its arguments before it asks for the device)"""
    dev, host = api._fn(NAMES[0]), api._fn(NAMES[1])
    return [lambda t, n, sps, iq, iq_len, off, ln, st, out: dev(None, t, n, sps, iq, off, ln, st, out),
            lambda t, n, sps, iq, iq_len, off, ln, st, out: host(t, n, sps, iq, iq_len, off, ln, st, out)]


def _args():
    iq = np.zeros(4096, np.complex64)
    return dict(iq=iq, off=np.zeros(1, np.uint64), ln=np.full(1, 4096, np.uint64), st=np.zeros(1, np.int32),
                out=np.zeros(1, np.dtype("V%d" % (24 + 192))))


def test_bad_arguments_are_refused(pkg):
    api = pkg.api
    a = _args()
    p = lambda k: a[k].ctypes.data
    good = dict(t=0, n=1, sps=4, iq=p("iq"), iq_len=4096, off=p("off"), ln=p("ln"), st=p("st"), out=p("out"))
    bad = [dict(t=-1), dict(t=3), dict(n=-1), dict(sps=0), dict(sps=17), dict(iq=None), dict(off=None), dict(ln=None),
           dict(out=None), dict(iq=p("iq") + 4)]
    for f in _calls(api):
        for change in bad:
            assert f(**dict(good, **change)) == -EINVAL, change
            assert b"fcch_acquire" in api._fn("gmr1_hip_last_error")()
    # the host form knows how long iq is and sees the arrays: a stream that leaves iq, a negative start
    host = _calls(api)[1]
    assert host(**dict(good, iq_len=4095)) == -EINVAL
    a["off"][0] = 1
    assert host(**good) == -EINVAL
    a["off"][0] = 0
    a["st"][0] = -1
    assert host(**good) == -EINVAL


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the calls would run")
def test_without_a_device_both_calls_say_so(pkg):
    api = pkg.api
    a = _args()
    p = lambda k: a[k].ctypes.data
    for f in _calls(api):
        assert f(0, 1, 4, p("iq"), 4096, p("off"), p("ln"), None, p("out")) == -ENODEV
    with pytest.raises(api.Gmr1HipError, match="-19"):
        api.fcch_acquire(a["iq"], [0], [4096])
