"""The per-device cache without HIP (osmo-gmr_amd/csrc/dev_cache.h): eight threads as eight devices ask for eleven keys each,
in their own order, several times -- make runs 88 times, every address stays and keeps its contents, a failed make leaves no
entry.  The checks are tests/c/dev_cache_host.cpp's.  Plain, under the address and undefined-behaviour sanitizers, and under
the thread sanitizer (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["-fno-omit-frame-pointer", "-g"]
VARIANTS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + COMMON,
            "tsan": ["-fsanitize=thread"] + COMMON}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_entries_are_made_once_and_stay_where_they_are(tmp_path, variant):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    obj, exe = str(tmp_path / "dev_cache_host.o"), str(tmp_path / "dev_cache_host")
    gxx = ["g++", "-std=c++17", "-O1", "-Wall", "-pthread"] + VARIANTS[variant]
    subprocess.check_call(gxx + ["-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"), "-c",
                                 os.path.join(ROOT, "tests", "c", "dev_cache_host.cpp"), "-o", obj])
    linked = subprocess.run(gxx + [obj, "-o", exe], capture_output=True, text=True)
    if variant == "tsan" and linked.returncode:
        pytest.skip("this toolchain cannot link the thread sanitizer's runtime")
    assert linked.returncode == 0, linked.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert res.returncode == 0 and res.stdout == "ok\n", res.stdout + res.stderr
