"""The fused batch kernel's packed per-lane operand tables without a GPU (osmo-gmr_amd/csrc/rx4_operands.h, compiled for the
host with host_tables.cpp): every ord4 entry against the ord_of_sym rows of the built-in BCCH / DC6 descriptors, every steps4
entry against the trellis-step descriptors worked out from the interleaver and the scrambler, both kinds and chains, all 64
lanes, all four places a lane, the -1 and 0 fills included; and the rule that refuses the fused path when a table is
perturbed (fused_operands_match, rx_select.h).  The checks are tests/c/rx4_operands_host.cpp's.  Once plain, once under the
address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


@pytest.mark.parametrize("extra", ([], SAN), ids=("plain", "asan_ubsan"))
def test_packed_tables_say_what_they_pack_and_the_refusal_fires(tmp_path, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "osmo-gmr_amd", "csrc")
    exe = str(tmp_path / "rx4_operands_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + extra +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "c", "rx4_operands_host.cpp"), os.path.join(csrc, "host_tables.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert res.returncode == 0 and res.stdout == "ok\n", res.stdout + res.stderr
