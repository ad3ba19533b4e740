"""Where k_rx4 touches the next burst's window (osmo-gmr_amd/csrc/rx_touch.h), checked on the CPU: a stand-alone program
built with the address and undefined-behaviour sanitizers reads every touched dword of every window length in
{960, 976, 1016, 1024} x every 8-byte start within a 128-byte line out of a heap block that ends with the window, and checks
that no address lies before the window or behind its last dword, that every line the window overlaps is touched and that
nothing is touched for a burst the wave does not take next (tests/c/rx4_touch_span.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in ("g++", "clang++"):
        if shutil.which(cxx):
            return cxx
    pytest.skip("no host C++ compiler")


def test_touch_addresses_stay_inside_the_window_and_cover_it(tmp_path):
    exe = str(tmp_path / "rx4_touch_span")
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "rx4_touch_span.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split()
    # 4 lengths x 16 starts; a window of L samples that starts s bytes into a line overlaps (s + 8 L - 1) // 128 + 1 lines
    want = sum((s + 8 * n - 1) // 128 + 1 for n in (960, 976, 1016, 1024) for s in range(0, 128, 8))
    assert out[0] == "OK" and int(out[1]) == want
