#!/usr/bin/env python3
"""Device-resident timing of the TCH9 call follower: gmr1_hip_tch9_follow_batch_dev over `calls` calls of `frames` frames
at sps 4, 9k6.  One synthesised CSD carrier of `frames` TCH9 bursts serves every call (each call has its own key and
state), so the windows are shared but every per-frame slot of the follower is its own.
GPU box, repo root: python3 tools/time_tch9_follow.py [calls [frames]]; per-kernel times: run it under
rocprofv3 --kernel-trace --stats."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
api, synth = pkg.api, pkg.synth
torch.cuda.init()
api.load()
api.init(0)
n_calls = int(sys.argv[1]) if len(sys.argv) > 1 else 256
n_fr = int(sys.argv[2]) if len(sys.argv) > 2 else 64
sps, tn, span = 4, 5, 5
rng = np.random.default_rng(1)
frame_len = 24 * 39 * sps
kc = rng.integers(0, 256, (n_calls, 8), dtype=np.uint8)
fn0 = 1000
ks = api.a5_batch(1, kc[0], np.arange(fn0, fn0 + n_fr), 658)
e = api.tch9_encode_batch(rng.integers(0, 256, (n_fr, 60), dtype=np.uint8), 2, n_fr, rng.integers(0, 2, (n_fr, 10), dtype=np.uint8),
                          rng.integers(0, 2, (n_fr, 4), dtype=np.uint8), ks)
body = synth.shape_bursts(synth.map_symbols(api.burst_format("nt9"), e, sync_id=1), sps, 0.0, span)
n = (n_fr + 1) * frame_len
x = (rng.standard_normal((n, 2)) * 0.03).astype(np.float32).view(np.complex64).reshape(-1)
for k in range(n_fr):
    pos = k * frame_len + tn * 39 * sps
    x[pos:pos + body.shape[1]] += body[k]
e_toa = (sps + sps // 2) >> 1
off1 = np.array([k * frame_len + tn * 39 * sps + span * sps - e_toa for k in range(n_fr)], np.uint64)

nt = n_calls * n_fr
state = np.zeros(n_calls, api.TCH9_STATE)
state["active"] = 1
state["kc"] = kc
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
t = dict(iq=dev(x), first=dev(np.arange(0, nt + 1, n_fr, dtype=np.int32)), offset=dev(np.tile(off1, n_calls)),
         fs=dev(np.zeros(nt, np.float32)), fn=dev(np.tile(np.arange(fn0, fn0 + n_fr, dtype=np.uint32), n_calls)), state=dev(state))
out = torch.zeros(nt * api.TCH9_FRAME.itemsize, dtype=torch.uint8, device="cuda")
state0 = t["state"].clone()
st = torch.cuda.current_stream().cuda_stream


def step():
    t["state"].copy_(state0)
    api.tch9_follow_dev(st, n_calls, nt, t["iq"].data_ptr(), t["first"].data_ptr(), t["offset"].data_ptr(), t["fs"].data_ptr(),
                        t["fn"].data_ptr(), t["state"].data_ptr(), out.data_ptr(), sps=sps)


for _ in range(5):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(20):
    step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / 20
rec = np.frombuffer(out.cpu().numpy().tobytes(), api.TCH9_FRAME)
print("%d calls x %d frames: %.3f ms per invocation, %.3f us per frame; classes %s, TCH9 frames of call 0: %d of %d" % (
    n_calls, n_fr, dt * 1e3, dt * 1e6 / nt, np.bincount(rec["cls"], minlength=4).tolist(),
    int((rec["cls"][:n_fr] == api.TCH9_TCH9).sum()), n_fr))
