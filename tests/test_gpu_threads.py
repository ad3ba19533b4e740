"""Several host threads on one device (reference deployment: one gmr1_rx process per carrier file in parallel,
utils/gmr1_process_recording.py:103-110).  The calls that share the library's per-device workspace take turns -- the host
part under a per-device lock, the device part ordered by an event across streams (csrc/capi_common.h: WsLease) -- so
concurrent callers get exactly what they get alone."""
import threading

import numpy as np
import pytest

import workloads

pytestmark = pytest.mark.gpu


def _key(rec):
    return [(int(r["arfcn"]), int(r["chain"]), int(r["type"]), int(r["fn"]), int(r["tn"]), bytes(r["l2"])) for r in rec]


@pytest.mark.timeout(600)
def test_two_threads_share_the_device_workspace(gpu_api, orc, pkg):
    import torch
    # thread A: receive loop over two carriers on its own stream; thread B: FCCH sweeps + a long detection list + the
    # two-launch TCH3 call on another stream -- all workspace users, sizes chosen so that the workspace GROWS mid-way
    carriers = [workloads.bcch_carrier(pkg, 300 + a, seconds=2.5, sps=4, stn=3 * a, delay=a, cfo_hz=50.0 * a)[0] for a in range(2)]
    ns = carriers[0].size
    d_car = torch.from_numpy(np.concatenate(carriers).view(np.float32)).cuda()
    want_rx = [_key(orc.rx_run(c, sps=4, arfcn=a)[1]) for a, c in enumerate(carriers)]
    fc = workloads.fcch_streams(pkg, 48, seed=9)
    want_toa = np.array([orc.fcch_rough(fc["iq"][i], 4)[1] for i in range(6)])
    d_fc = torch.from_numpy(fc["iq"].view(np.float32)).cuda()
    d_fo = torch.from_numpy(fc["offset"].astype(np.int64)).cuda()
    nt = workloads.nt3_mix(pkg, 400, seed=3)
    sp = nt["speech"][:300]
    alone = gpu_api.tch3_rx_batch(nt["iq"], nt["offset"][sp], 474, sps=4, freq_shift=nt["freq_shift"][sp], want_ebits=False)
    errs, out = [], {}
    go = threading.Barrier(2)

    def thread_a():
        try:
            st = torch.cuda.Stream()
            go.wait()
            for it in range(6):
                rec, status, chains, found = gpu_api.rx_run_dev(st.cuda_stream, d_car.data_ptr(), [0, ns], [ns, ns], sps=4)
                assert not status.any()
                for a in range(2):
                    assert _key(rec[rec["arfcn"] == a]) == [(a,) + k[1:] for k in want_rx[a]], f"iteration {it}, carrier {a}"
            out["a"] = True
        except BaseException as e:      # noqa: BLE001 - reported by the main thread
            errs.append(("a", repr(e)))

    def thread_b():
        try:
            st = torch.cuda.Stream()
            toa = torch.zeros(48, dtype=torch.int32, device="cuda")
            rv = torch.zeros(48, dtype=torch.int32, device="cuda")
            go.wait()
            for it in range(6):
                n = 8 * (it + 1)                                     # growing batches: the workspace is re-allocated
                gpu_api.fcch_rough_batch_dev(st.cuda_stream, "fcch", n, 4, fc["n_samples"], d_fc.data_ptr(), d_fo.data_ptr(), None,
                                             toa.data_ptr(), rv.data_ptr())
                st.synchronize()
                assert np.array_equal(toa.cpu().numpy()[:6], want_toa), f"iteration {it}"
                got = gpu_api.tch3_rx_batch(nt["iq"], nt["offset"][sp], 474, sps=4, freq_shift=nt["freq_shift"][sp], want_ebits=False)
                for k in ("frame0", "frame1", "rv", "toa"):
                    assert np.array_equal(got[k], alone[k]), (it, k)
            out["b"] = True
        except BaseException as e:      # noqa: BLE001
            errs.append(("b", repr(e)))

    ts = [threading.Thread(target=thread_a), threading.Thread(target=thread_b)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(500)
    assert not errs, errs
    assert out.get("a") and out.get("b")


def test_four_threads_make_their_first_transmit_calls_together(gpu_api, orc, pkg):
    """Four threads leave a barrier into four different calls, each of which asks a per-device cache (csrc/dev_cache.h) for a
    table it builds and uploads on first use: a BCCH encoder plan, the TCH9 9k6 plan, the BCCH format's modulator tables, an
    NT9 gather map.  Run alone, these are the process's first such calls, so the four builds race; within the suite the
    lookups do.  Every result is what the oracle gives; the shaped windows lie within test_gpu_mod_shaped's derived bound of
    its float64 restatement over the oracle's symbols."""
    from test_gpu_mod_shaped import restate
    rng = np.random.default_rng(41)
    l2_b = rng.integers(0, 256, (5, 24), dtype=np.uint8)
    l2_t = rng.integers(0, 256, (6, 60), dtype=np.uint8)
    sa, stt = rng.integers(0, 2, (6, 10), dtype=np.uint8), rng.integers(0, 2, (6, 4), dtype=np.uint8)
    ciph = rng.integers(0, 2, (6, 658), dtype=np.uint8)
    info = gpu_api.burst_info("bcch")
    bits = rng.integers(0, 2, (3, info.ebits), dtype=np.uint8)
    sps, span, in_len = 4, 4, info.len * 4 + 16
    start = np.array([8, 6, 10], np.int32)
    l2_d = rng.integers(0, 256, (6, 30), dtype=np.uint8)
    c_d = rng.integers(0, 2, (6, 658), dtype=np.uint8)
    hard = np.concatenate([orc.tch9_encode_seq(l2_d[r:r + 3], 1, sa[r:r + 3], stt[r:r + 3], c_d[r:r + 3]) for r in (0, 3)])
    eb = (127 * (1 - 2 * hard.astype(np.int16))).astype(np.int8)
    with gpu_api.conv_decoder(gpu_api.CONV_GENERIC), orc.conv_mode(0):
        want = {
            "bcch": orc.bcch_encode(l2_b),
            "tch9": np.concatenate([orc.tch9_encode_seq(l2_t[r:r + 3], 2, sa[r:r + 3], stt[r:r + 3], ciph[r:r + 3]) for r in (0, 3)]),
            "nt9": [np.concatenate([orc.tch9_decode_seq(eb[r:r + 3], 1, c_d[r:r + 3])[k] for r in (0, 3)]) for k in range(4)],
        }
        sym = np.stack([orc.mod("bcch", bits[i], 0) for i in range(3)])
        shaped, bound = restate(pkg.synth, sym, sps, in_len, "rc", span, start=start)
        calls = {
            "bcch": lambda: gpu_api.bcch_encode_batch(l2_b),
            "tch9": lambda: gpu_api.tch9_encode_batch(l2_t, 2, 3, sa, stt, ciph),
            "mod": lambda: gpu_api.mod_shaped_batch("bcch", bits, sps, in_len, span=span, start=start),
            "nt9": lambda: gpu_api.tch9_decode_batch(eb, 1, 3, c_d),
        }
        go = threading.Barrier(len(calls))
        got, errs = {}, []

        def run(name):
            try:
                go.wait()
                got[name] = calls[name]()
            except BaseException as e:      # noqa: BLE001 - reported by the main thread
                errs.append((name, repr(e)))

        ts = [threading.Thread(target=run, args=(name,)) for name in calls]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
    assert not errs, errs
    assert sorted(got) == sorted(calls)
    assert np.array_equal(got["bcch"], want["bcch"])
    assert np.array_equal(got["tch9"], want["tch9"])
    assert np.array_equal(want["nt9"][0][2::3], l2_d[0::3]), "the oracle's own decode gives back what was sent"
    for g, w in zip(got["nt9"], want["nt9"]):
        assert np.array_equal(g, w)
    assert bound.max() > 0 and not got["mod"][bound == 0].any()
    assert (np.abs(got["mod"].astype(np.complex128) - shaped) <= bound).all()
