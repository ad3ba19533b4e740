"""The streaming channelizer's entry points without a GPU: like every compute entry point, they fail loudly (-ENODEV)."""
import ctypes as C

import pytest


def test_chan_stream_without_gpu_is_enodev(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.ChanStream(2.0e6, [5, 40])
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.ChanStream.direct(2.0e6, [31250.0])
    lib = pkg.api.load()
    n = C.c_uint64()
    assert lib.gmr1_hip_chan_stream_out_len(None, C.c_uint64(100), C.byref(n)) == -19
    assert lib.gmr1_hip_chan_stream_push(None, None, C.c_uint64(0), None, C.c_uint64(0), C.byref(n)) == -19
    assert lib.gmr1_hip_chan_stream_push_dev(None, None, None, C.c_uint64(0), None, C.c_uint64(0), C.byref(n)) == -19
    assert lib.gmr1_hip_chan_stream_destroy(None) == -19
