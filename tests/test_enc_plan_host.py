"""The encoder plan builder without the library or a GPU (osmo-gmr_amd/csrc/enc_plan.cpp, compiled with plain g++ and no ROCm
include path): all 11 chains built twice and byte-equal, the sizes the public header and the plan_* functions state, every
descriptor of out[] and ext_src[] within what k_encode indexes.  The checks are tests/c/enc_plan_host.cpp's.  Once plain, once
under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


@pytest.mark.parametrize("extra", ([], SAN), ids=("plain", "asan_ubsan"))
def test_every_plan_is_whole_and_in_range(tmp_path, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "osmo-gmr_amd", "csrc")
    exe = str(tmp_path / "enc_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + extra +
                          ["-I" + csrc, os.path.join(ROOT, "tests", "c", "enc_plan_host.cpp"), os.path.join(csrc, "enc_plan.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert res.returncode == 0 and res.stdout == "ok\n", res.stdout + res.stderr
