"""The streaming receive loop without a GPU (every entry point -ENODEV), and its arithmetic (osmo-gmr_amd/csrc/rx_stream.h,
compiled for the host): when the acquisition may run, what a carrier keeps, when a stopped chain resumes."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rx_stream_without_gpu_is_enodev(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.RxStream(4, sps=4)
    lib = pkg.api.load()
    h = C.c_void_p()
    m = C.c_int()
    assert lib.gmr1_hip_rx_stream_create(C.c_int(4), C.c_int(4), None, C.byref(h)) == -19
    assert lib.gmr1_hip_rx_stream_max_records(None, C.c_uint64(100), C.byref(m)) == -19
    assert lib.gmr1_hip_rx_stream_push_dev(None, None, None, C.c_uint64(0), C.c_uint64(0), C.c_int(1), None, C.c_int(0),
                                           C.byref(m)) == -19
    assert lib.gmr1_hip_rx_stream_push(None, None, C.c_uint64(0), C.c_uint64(0), C.c_int(1), None, C.c_int(0),
                                       C.byref(m)) == -19
    assert lib.gmr1_hip_rx_stream_status(None, None, None, None) == -19
    assert lib.gmr1_hip_rx_stream_destroy(None) == -19


PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "rx_stream.h"
using namespace gmr1;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)
int main()
{
    for (int sps = 1; sps <= 16; sps++) {
        const long long wl1 = 330LL * 23400 * sps / 1000, wl3 = 650LL * 23400 * sps / 1000, flen = 117LL * sps;
        const int fl = rx_stream_frame_len(sps);
        CHECK(fl == 936 * sps);
        // H_acq: the start discard, both sweep windows and three FCCH bursts.  This restates the formula; that it is large
        // enough for RxRun::acquire rests on the derivation in rx_stream.h (the ranges of the sweeps' results, checked
        // below as far as they are arithmetic) and on the GPU tests of captures ending around H_acq
        CHECK(rx_stream_acq_need(sps) == 8000 + wl1 + wl3 + 3 * flen);
        // ... covers every end the acquisition compares: the rough toa <= wl1 - flen, |fine toa| < flen, peaks <= wl3 - flen
        const long long worst = 8000 + (wl1 - flen) + flen - flen + (wl3 - flen) + flen + flen;
        CHECK(worst <= rx_stream_acq_need(sps));
        // the fine stage's largest offset: 116 bins / 2 of 200 Hz over the chirp rate, in samples
        const double chirp = 2.0 * 0.32 * 23400.0 * 23400.0 / (117.0 * 1000.0);
        CHECK((116.0 * 200.0 / 2.0) / chirp * 23400.0 * sps / 1000.0 < flen);
        // retention: the margin kept before a chain covers the farthest a window can reach back
        CHECK(2 * fl > rx_stream_reach_back(sps));
        for (long long a = 0; a < 20 * fl; a += 97) {
            const long long k = rx_stream_keep_from(a, sps);
            CHECK(k >= 0 && k % kRxKeepAlign == 0 && k <= a);
            CHECK(a - k < 2 * fl + kRxKeepAlign);
            CHECK(a < 2 * fl || a - k >= 2 * fl);
            CHECK(a < 2 * fl || a - k >= rx_stream_reach_back(sps));
            // a chain stopped at a (a + 2 fl > H) leaves the carrier holding fewer than 4 frame lengths + 64
            const long long H = a + 2 * fl - 1;
            CHECK(H - k < 4 * fl + kRxKeepAlign);
        }
        // release rules
        CHECK(rx_stream_next_done(kRxDoneUnstarted, 5000, 5000 + 2 * fl, sps, 0) == 0);
        CHECK(rx_stream_next_done(kRxDoneUnstarted, 5000, 5000 + 2 * fl - 1, sps, 0) == kRxDoneUnstarted);
        CHECK(rx_stream_next_done(kRxDoneUnstarted, 5000, 5000 + 2 * fl - 1, sps, 1) == 0);
        CHECK(rx_stream_next_done(kRxDoneStopped, 5000, 5000 + 2 * fl, sps, 0) == 0);
        CHECK(rx_stream_next_done(kRxDoneStopped, 5000, 5000 + 2 * fl - 1, sps, 1) == kRxDoneStopped);
        CHECK(rx_stream_next_done(kRxDoneFinal, 0, 1 << 30, sps, 1) == kRxDoneFinal);
        // the record bound is the loop's per-chain buffer, and a chain emits at most one record per frame it walks
        for (long long len = 0; len < 50LL * fl; len += 1013)
            CHECK(rx_stream_rec_per_chain(len, sps) >= len / fl + 2);
    }
    std::printf("ok\n");
    return 0;
}
"""


def test_rx_stream_arithmetic(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "rx_stream_host.cpp"
    src.write_text(PROG)
    exe = str(tmp_path / "rx_stream_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"), str(src), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
