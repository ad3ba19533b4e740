"""Channelizer host-code A/B, one library per run (GMR1_HIP_LIBRARY; unset: the product build), for refactors of
capi_chan.cpp / capi_chan_stream.cpp / chan_plan.h that must leave every output and time as it was:

    GMR1_HIP_LIBRARY=.../libgmr1_hip_X.so python tools/exp/chan_ab_outputs.py hash   # sha256 of the existing tests' seeded
        captures: one-shot, planar and streamed with the "random" schedule; filterbank on and off the grid, direct mode with
        both banks.  Two libraries agree when their outputs are the same text.
    GMR1_HIP_LIBRARY=.../libgmr1_hip_X.so python tools/exp/chan_ab_outputs.py push   # wall time per push_dev of the capture of
        test_filterbank_fast_path_streams_bit_identically in equal pushes (6 x 100000 + 7), one stream, 300 passes
"""
import hashlib
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
torch.cuda.init()
from __graft_entry__ import load_package
api = load_package().api
api.load(); api.init(0)
import test_gpu_chan_stream as ts

def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

def streamed(cs, x, sizes):
    outs, pos = [], 0
    for k in sizes:
        outs.append(cs.push(x[pos:pos + k])); pos += k
    return np.concatenate(outs, axis=1)

def hashes():
    n = 600007
    x = ts._capture(n, 2.0e6, 11)
    for sps in (1, 3, 4, 13):
        print("oneshot chan 2.000 sps %d" % sps, h(api.channelize(x, 2.0e6, ts.CHANS, sps=sps)))
    print("oneshot chan 2.000 sps 4 rot", h(api.channelize(x, 2.0e6, ts.CHANS, rotation=0.21)))
    with api.ChanStream(2.0e6, ts.CHANS) as cs:
        print("stream  chan 2.000 sps 4 random", h(streamed(cs, x, ts._random_sizes(n, 12))))
    with api.ChanStream(2.0e6, ts.CHANS, sps=1) as cs:
        print("stream  chan 2.000 sps 1 random", h(streamed(cs, x, ts._random_sizes(n, 12))))
    # planar, sps 4 and 3 (device entry)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    xd = torch.from_numpy(x.view(np.float32).reshape(-1, 2).copy()).to(dev)
    for sps in (4, 3):
        _, _, n_out = api.channelize_plan(2.0e6, sps, n)
        stride = n_out
        plane = -(-len(ts.CHANS) * stride // sps)
        out = torch.zeros((sps, plane, 2), device=dev, dtype=torch.float32)
        api.channelize_planar_dev(st.cuda_stream, xd.data_ptr(), n, 2.0e6, ts.CHANS, out.data_ptr(), stride, plane, sps=sps)
        torch.cuda.synchronize()
        print("planar  chan 2.000 sps %d" % sps, h(out.cpu().numpy()))
    for fs in (2.048e6, 1.25e6, 2.4e6):
        M, _, _ = api.channelize_plan(fs, 4, 0)
        nn = 40 * M * 50 + 37
        xx = ts._capture(nn, fs, int(fs) % 1000 + 5, M)
        chans = [3, M - 2, M // 2 - 1, 0, M - 1, M // 2]
        for rot in (0.0, 0.21):
            print("oneshot chan %.3f rot %.2f" % (fs / 1e6, rot), h(api.channelize(xx, fs, chans, rotation=rot)))
            with api.ChanStream(fs, chans, rotation=rot) as cs:
                print("stream  chan %.3f rot %.2f random" % (fs / 1e6, rot), h(streamed(cs, xx, ts._random_sizes(nn, int(fs) % 77, hi=nn // 5))))
    freqs = [3 * 31250.0, -7 * 31250.0 + 400.0, 0.0]
    nd = 200013
    for fs in (2.0e6, 1.25e6, 2.5e6, 4.0e6, 1.0e6):
        xx = ts._capture(nd, fs, int(fs) % 97)
        for sps in (2, 4):
            print("oneshot ddc  %.3f sps %d" % (fs / 1e6, sps), h(api.ddc(xx, fs, freqs, sps=sps)))
            with api.ChanStream.direct(fs, freqs, sps=sps) as cs:
                print("stream  ddc  %.3f sps %d random" % (fs / 1e6, sps), h(streamed(cs, xx, ts._random_sizes(nd, 3, hi=40000))))

def push_time():
    n = 600007
    x = ts._capture(n, 2.0e6, 11)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    xd = torch.from_numpy(x.view(np.float32).reshape(-1, 2).copy()).to(dev)
    sizes = [100000] * 6 + [7]
    out = torch.zeros((len(ts.CHANS), 200000, 2), device=dev, dtype=torch.float32)
    with api.ChanStream(2.0e6, ts.CHANS) as cs:
        def one_pass():
            pos = 0
            for k in sizes:
                cs.push_dev(st.cuda_stream, xd.data_ptr() + 8 * pos, k, out.data_ptr(), 200000)
                pos += k
            torch.cuda.synchronize()
        t_end = time.perf_counter() + 0.5
        while time.perf_counter() < t_end:
            one_pass()
        ts_ = []
        for _ in range(300):
            t0 = time.perf_counter(); one_pass(); ts_.append((time.perf_counter() - t0) / len(sizes) * 1e6)
    ts_ = np.array(ts_)
    print("push_us_median %.3f p10 %.3f p90 %.3f" % (np.median(ts_), np.percentile(ts_, 10), np.percentile(ts_, 90)))

if sys.argv[1] == "hash":
    hashes()
else:
    push_time()
