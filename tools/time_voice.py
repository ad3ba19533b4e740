#!/usr/bin/env python3
"""Device-resident timing of the speech decoder's calls entry (gmr1_hip_tch3_frames_to_pcm_dev) against the dense entry
(gmr1_hip_codec_decode_batch_dev) on the same frames, in one process, the two alternating (no copies in the timed
region; device events).  Shape: the AMBE side workload's, 8192 calls x 50 all-speech records = 819 200 frames.  Then the
calls entry again with every second record not speech, and the audio entry (gmr1_hip_tch3_frames_to_audio_dev: the close-up
kernel and the decoder's audio instantiation, samples into 656-byte blocks) on the all-speech records.  Run by hand on the
GPU: time_voice.py [calls] [records] [rounds]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
api = pkg.api
torch.cuda.init()
api.load()
api.init(0)
n_calls = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
n_rec = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 15
LAUNCHES = 10                                   # per timed window: ~0.1 s of work at the default shape
n_frames = 2 * n_rec
stream = torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


frames = pkg.synth.ambe_speech_frames(n_calls, n_frames, seed=7)
rec = np.zeros((n_calls, n_rec), api.TCH3_FRAME)
rec["cls"], rec["type"], rec["len"] = api.TCH3_SPEECH, 0x10, 20
rec["l2"] = frames.reshape(n_calls, n_rec, 20)
half = rec.copy()
half["type"][:, 1::2] = 0                       # every second record is what a DKAB frame leaves: no payload
half["cls"][:, 1::2] = api.TCH3_DKAB
first = np.arange(n_calls + 1, dtype=np.int32) * n_rec

d_frames, d_rec, d_half, d_first = dev(frames), dev(rec), dev(half), dev(first)
d_state = torch.zeros((n_calls, api.codec_state_bytes()), dtype=torch.uint8, device="cuda")
d_pcm = torch.zeros((n_calls * n_frames, 160), dtype=torch.int16, device="cuda")
d_pcm2 = torch.zeros_like(d_pcm)
d_rv = torch.zeros(n_calls * n_frames, dtype=torch.int32, device="cuda")


def dense(pcm=d_pcm):
    api.codec_decode_batch_dev(stream, n_calls, n_frames, d_frames.data_ptr(), pcm.data_ptr(), d_rv.data_ptr(), d_state.data_ptr())


def calls_on(records):
    def run(pcm=d_pcm):
        api.tch3_frames_to_pcm_dev(stream, n_calls, n_calls * n_rec, d_first.data_ptr(), records.data_ptr(), d_state.data_ptr(),
                                   pcm.data_ptr(), d_rv.data_ptr())
    return run


calls_all, calls_half = calls_on(d_rec), calls_on(d_half)
d_audio = torch.zeros((n_calls * n_rec, api.RX_AUDIO.itemsize), dtype=torch.uint8, device="cuda")
d_fn = torch.arange(n_calls * n_rec, dtype=torch.int32, device="cuda")
d_label = dev(np.array([api.tch3_audio_label(c & 0xffff, c >> 16, 0, 1) for c in range(n_calls)], np.uint64))
d_found = torch.zeros(1, dtype=torch.int32, device="cuda")


def audio():
    api.tch3_frames_to_audio_dev(stream, n_calls, n_calls * n_rec, d_first.data_ptr(), d_rec.data_ptr(), d_fn.data_ptr(),
                                 d_label.data_ptr(), d_state.data_ptr(), d_audio.data_ptr(), n_calls * n_rec, d_found.data_ptr())



def fresh():
    api.codec_init_dev(stream, n_calls, d_state.data_ptr())


def window(step):
    """LAUNCHES launches from fresh decoders -> milliseconds per launch"""
    fresh()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES


# the two entries compute the same samples and states on these frames: faster and different would not be faster
fresh()
dense(d_pcm)
s_dense = d_state.clone()
fresh()
calls_all(d_pcm2)
torch.cuda.synchronize()
assert torch.equal(d_pcm, d_pcm2) and torch.equal(s_dense, d_state), "the calls entry and the dense entry differ"

fresh()
audio()
torch.cuda.synchronize()
blocks = d_audio.view(torch.int16).reshape(n_calls * n_rec, -1)
assert int(d_found[0]) == n_calls * n_rec and torch.equal(blocks[:, 8:].reshape(-1, 160), d_pcm) and torch.equal(s_dense, d_state), \
    "the audio entry and the dense entry differ"

steps = {"dense": dense, "calls": calls_all, "calls_half_speech": calls_half, "audio": audio}
for step in steps.values():                     # warm-up: every shape the timed windows use
    window(step)
ms = {k: [] for k in steps}
for _ in range(rounds):                         # alternating, so that drift of the clock or the host hits all alike
    for k, step in steps.items():
        ms[k].append(window(step))

res = {"n_calls": n_calls, "records_per_call": n_rec, "frames": n_calls * n_frames, "rounds": rounds, "launches_per_window": LAUNCHES}
for k, v in ms.items():
    v = np.array(v)
    res[k] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
              "spread_ms": float(v.max() - v.min())}
    print("%-18s median %.3f ms, min %.3f, max %.3f (spread %.3f) per launch" %
          (k, res[k]["median_ms"], v.min(), v.max(), v.max() - v.min()))
d, c, h = (res[k]["median_ms"] for k in ("dense", "calls", "calls_half_speech"))
res["calls_minus_dense_ms"] = c - d
res["audio_minus_calls_ms"] = res["audio"]["median_ms"] - c
res["frames_per_s_dense"] = n_calls * n_frames / (d * 1e-3)
res["frames_per_s_calls"] = n_calls * n_frames / (c * 1e-3)
# every call has the same records, so the launch's time divides by record position: a position that is not speech costs what
# is left when half of the positions are taken out of the decoder
res["us_per_speech_position"] = c * 1e3 / n_rec
res["us_per_zero_position"] = (h - c / 2) * 1e3 / (n_rec / 2)
print("calls - dense: %+.3f ms (%.2f %% of dense; spread of dense %.3f ms)" % (c - d, 100 * (c - d) / d, res["dense"]["spread_ms"]))
print("audio - calls: %+.3f ms (%.2f %% of calls; spread of calls %.3f ms)" %
      (res["audio_minus_calls_ms"], 100 * res["audio_minus_calls_ms"] / c, res["calls"]["spread_ms"]))
print("of the launch's time, a record position takes %.1f us where it is speech and %.2f us where it is not" %
      (res["us_per_speech_position"], res["us_per_zero_position"]))
print(json.dumps(res))
