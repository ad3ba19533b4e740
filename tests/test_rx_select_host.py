"""The host's kernel-choice and fused-path rules without a GPU (osmo-gmr_amd/csrc/rx_select.h, compiled for the host with
host_tables.cpp): which demodulation kernel a batch of each built-in format gets at which window, what the fused BCCH / DC6
path asks of the burst tables, its window lengths, staging size and kernel choice -- against the values written down in
tests/c/rx_select_host.cpp.  On a GPU a wrong choice leaves every output correct and only moves a time, so nothing else
notices.  Once plain, once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is
preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
BUILDS = pytest.mark.parametrize("extra", ([], SAN), ids=("plain", "asan_ubsan"))


def run_rx_select_host(tmp_path, extra, args=()):
    """tests/c/rx_select_host.cpp built with the compiler flags `extra` and run with `args` -> the lines it printed; its
    own checks ran first, and the last line is their "ok" """
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "osmo-gmr_amd", "csrc")
    exe = str(tmp_path / "rx_select_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + extra +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "c", "rx_select_host.cpp"), os.path.join(csrc, "host_tables.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env)
    lines = res.stdout.split("\n")
    assert res.returncode == 0 and lines[-2:] == ["ok", ""], res.stdout + res.stderr
    return lines[:-2]


@BUILDS
def test_kernel_choice_and_fused_rules_on_the_builtin_tables(tmp_path, extra):
    assert run_rx_select_host(tmp_path, extra) == []
