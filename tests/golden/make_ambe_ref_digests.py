#!/usr/bin/env python3
"""Writes tests/golden/ambe_ref_digests.npz: what the reference's vocoder, built from its sources (tests/ref_codec.py), gives
for the fresh streams of tests/test_oracle_ambe.py, as one 64-bit digest per 160-sample frame (needs the sources).  Per key
("s<seed>_<k>" for stream k of fresh_streams(seed), "rejected" for the stream with invalid tone codes):
    <key>_frames_digest  [n] uint64   the input frames (a changed stream generator is caught, not compared)
    <key>_clean          [n] uint64   gmr1_codec_decode_frame entered on a zeroed stack
    <key>_rv             [n] int32    its return values
    <key>_pcm            [n] uint64   the reference's program gmr1_ambe_decode on the same file (not for "rejected")
and per family of aimed streams (tests/ambe_aimed.py; T.aimed_streams(): "orbit", "histories", "levels", "tones"), over its
channels one after the other, every channel on a decoder of its own:
    aimed_<family>_frames_digest  uint64   the input frames, one digest per 16 frames of a channel
    aimed_<family>_clean          uint64   gmr1_codec_decode_frame entered on a zeroed stack: one digest per frame, for
                                           "histories" (61 752 frames) one per 16 frames of a channel (T.AIMED_BLOCK)
    aimed_<family>_rv             int32    its return values, per frame
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_codec             # noqa: E402
import test_oracle_ambe as T     # noqa: E402

if not ref_codec.available():
    sys.exit("needs the reference's sources (tests/ref_codec.py)")
out = {}
jobs = [("s%d_%d" % (seed, k), fr, True) for seed in T.SEEDS for k, fr in enumerate(T.fresh_streams(seed))]
jobs.append(("rejected", T.rejected_tone_stream(), False))
for key, fr, program in jobs:
    clean, rv, prog = T.reference_outputs(key, fr, program)
    out[key + "_frames_digest"] = T.frame_digests(fr)
    out[key + "_clean"] = T.frame_digests(clean)
    out[key + "_rv"] = rv.astype(np.int32)
    if program:
        assert len(prog) == len(fr)
        out[key + "_pcm"] = T.frame_digests(prog)
for key, chans in T.aimed_streams().items():
    clean, rv = T.aimed_reference(key)
    out["aimed_%s_frames_digest" % key] = T.block_digests(chans, T.AIMED_FRAMES_BLOCK)
    out["aimed_%s_clean" % key] = T.block_digests(clean, T.AIMED_BLOCK[key])
    out["aimed_%s_rv" % key] = rv.astype(np.int32)
np.savez_compressed(os.path.join(HERE, "ambe_ref_digests.npz"), **out)
print("wrote", os.path.join(HERE, "ambe_ref_digests.npz"), os.path.getsize(os.path.join(HERE, "ambe_ref_digests.npz")), "bytes")
