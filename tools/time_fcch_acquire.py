"""Time per call of gmr1_hip_fcch_acquire_batch_dev next to the FCCH step bench.py --workload fcch times (the rough and fine
calls with torch element-wise kernels between them), both on workloads.fcch_streams, everything resident on the device.
The new call does more per stream (five sweeps and the decisions against two sweeps and no decision); the comparison says
what a caller pays for the whole acquisition against the part of it that could be had before.
    python tools/time_fcch_acquire.py [streams] [calls]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from __graft_entry__ import load_package
import workloads
torch.cuda.init()
pkg = load_package(); api = pkg.api; api.load(); api.init(0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
sps = 4
wl = workloads.fcch_streams(pkg, n, seed=2)
ns = wl["n_samples"]
iq = torch.from_numpy(wl["iq"].view(np.float32)).cuda()
offset = torch.from_numpy(wl["offset"].astype(np.int64)).cuda()
length = torch.full((n,), ns, dtype=torch.int64, device="cuda")
start = torch.zeros(n, dtype=torch.int32, device="cuda")      # 1-s streams: the 650 ms window fits from wherever the first burst is
out = torch.zeros(n * api.FCCH_ACQ.itemsize, dtype=torch.uint8, device="cuda")
toa = torch.zeros(n, dtype=torch.int32, device="cuda"); rv = torch.zeros(n, dtype=torch.int32, device="cuda")
ftoa = torch.zeros(n, dtype=torch.int32, device="cuda"); ferr = torch.zeros(n, dtype=torch.float32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
f_fine = api.load().gmr1_hip_fcch_fine_batch_dev; f_fine.restype = C.c_int

def acquire():
    api.fcch_acquire_dev(st, n, iq.data_ptr(), offset.data_ptr(), length.data_ptr(), out.data_ptr(), sps=sps, start=start.data_ptr())

def bench_step():
    api.fcch_rough_batch_dev(st, "fcch", n, sps, ns, iq.data_ptr(), offset.data_ptr(), None, toa.data_ptr(), rv.data_ptr())
    off_f = offset + torch.clamp(toa.to(torch.int64), 0, ns - 117 * sps)
    rc = f_fine(C.c_void_p(st), C.c_int(0), C.c_int(n), C.c_int(sps), C.c_void_p(iq.data_ptr()), C.c_void_p(off_f.data_ptr()), None,
                C.c_void_p(ftoa.data_ptr()), C.c_void_p(ferr.data_ptr()))
    assert rc == 0

def timed(f):
    for _ in range(5): f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls): f()
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return t_host / calls * 1e3, (time.perf_counter() - t0) / calls * 1e3

for name, f in (("gmr1_hip_fcch_acquire_batch_dev", acquire), ("rough + torch glue + fine (bench.py's fcch step)", bench_step)):
    host, whole = timed(f)
    print("%s: %.3f ms per call (%.3f ms of it on the host), %d streams of %d samples" % (name, whole, host, n, ns))
rec = np.frombuffer(out.cpu().numpy().tobytes(), api.FCCH_ACQ)
print("acquired: %d of %d streams, %d chains" % (int((rec["status"] == 0).sum()), n, int(rec["n_chains"].sum())))
