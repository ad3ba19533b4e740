"""The integer rules of the receive loop's traffic follow-ups without a GPU (osmo-gmr_amd/csrc/rx_follow.h, compiled for the
host): which frames of which chain belong to which TCH3 assignment and invocation, what a push carries in, when a missing
window is an error, and how a chain's NT9 bursts split into FACCH9 jobs and TCH9 interleaver runs -- by the one-shot
call's planner, and by tch9_plan_push with nothing carried in followed by the call follower's routing
(osmo-gmr_amd/csrc/tch9_follow.h) over every segment: which NT9 frames are mapped, which are FACCH9, TCH9 or failed, and
which two earlier TCH9 bursts of its interleaver run a TCH9 frame reads -- against the reference's
frame-by-frame rule restated in tests/c/rx_follow_host.cpp and tests/c/rx_tch9_ref.h, at sps 1, 4 and 16.  Once plain, once under the address and
undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


@pytest.mark.parametrize("extra", ([], SAN), ids=("plain", "asan_ubsan"))
def test_follow_up_plans_are_the_references_frame_loop(tmp_path, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "rx_follow_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra +
                          ["-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "rx_follow_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
