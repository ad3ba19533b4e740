"""Captures and helpers of tests/test_gpu_rx_stream_tch.py: BCCH carriers with the traffic carrier their IMMEDIATE
ASSIGNMENTs point to, the push loop of a handle that follows TCH3 calls, and the one-shot reference, computed once per
capture and Viterbi decoder mode and shared by the tests."""
import functools

import numpy as np

import workloads

SPS = 4
SECONDS = 4.0          # the shortest capture in which acquisition (about 1 s) leaves room for an assignment and a few dozen call frames
REASSIGNED = [(31, [(15, 11, 20), (55, 4, 7)]), (32, [(12, 20, 33), (40, 9, 12), (70, 11, 20)])]     # test_gpu_rxloop.py's


@functools.lru_cache(maxsize=1)
def pairs(pkg):
    """-> dict(x (5, n), t (5, n) complex64, kc (5, 8), ciphered: carrier -> the FACCH3 messages sent ciphered).  Four
    bcch_tch_pair carriers of equal length and a fifth whose traffic side is noise."""
    rng = np.random.default_rng(77)
    cases = [
        dict(seed=5, kc=np.array([1, 2, 3, 4, 5, 6, 7, 8], np.uint8), cipher_after=30),
        dict(seed=6, kc=None, cipher_after=None, tn=4, p=7, stn=1, delay=6),
        dict(seed=7, kc=rng.integers(0, 256, 8, dtype=np.uint8), cipher_after=0, tn=20, p=33, mix=(0.2, 0.3, 0.5)),
        dict(seed=8, kc=None, cipher_after=None, tn=9, p=12, k_stop=45),
    ]
    x, t, kcs, ciphered = [], [], [], {}
    for i, cs in enumerate(cases):
        cs = dict(cs)
        b, tr, _, sent_t = workloads.bcch_tch_pair(pkg, cs.pop("seed"), seconds=SECONDS, sps=SPS, **cs)
        x.append(b)
        t.append(tr)
        kcs.append(cs["kc"] if cs["kc"] is not None else np.zeros(8, np.uint8))
        if cs["kc"] is not None:
            ciphered[i] = {bytes(s["l2"]) for s in sent_t if s["type"] == "facch3" and s["ciph"]}
    b, _, _, _ = workloads.bcch_tch_pair(pkg, 9, seconds=SECONDS, sps=SPS)
    x.append(b)
    t.append((rng.standard_normal((b.size, 2)) * 0.05).astype(np.float32).view(np.complex64).reshape(-1))
    kcs.append(np.zeros(8, np.uint8))
    assert len({v.size for v in x + t}) == 1
    return dict(x=np.stack(x).astype(np.complex64), t=np.stack(t).astype(np.complex64), kc=np.stack(kcs), ciphered=ciphered)


@functools.lru_cache(maxsize=1)
def reassigned(pkg):
    """Two carriers whose calls are re-assigned once and twice, ciphered from 20 frames after the first assignment, at one
    common length -> dict(x, t, kc, ia: the assignments per carrier)"""
    kc = np.arange(1, 9, dtype=np.uint8)
    caps = [workloads.bcch_tch_reassigned(pkg, seed, ia, seconds=5.0, sps=SPS, kc=kc, cipher_after=20) for seed, ia in REASSIGNED]
    assert len({c[0].size for c in caps} | {c[1].size for c in caps}) == 1
    return dict(x=np.stack([c[0] for c in caps]).astype(np.complex64), t=np.stack([c[1] for c in caps]).astype(np.complex64),
                kc=np.stack([kc, kc]), ia=[ia for _, ia in REASSIGNED])


_ONE_SHOT = {}


def one_shot(api, name, cap, arfcn):
    """gmr1_hip_rx_run_tch on the whole capture, once per (capture, decoder mode) -> (records, status, chains)"""
    key = (name, api.get_conv_decoder(), bytes(np.asarray(arfcn, np.uint16)))
    if key not in _ONE_SHOT:
        A, n = cap["x"].shape
        offset = np.arange(A, dtype=np.uint64) * np.uint64(n)
        length = np.full(A, n, np.uint64)
        rec, status, chains, found = api.rx_run_tch(cap["x"].reshape(-1), cap["t"].reshape(-1), offset, length, sps=SPS, arfcn=arfcn,
                                                    kc=cap["kc"], max_records=1 << 20)
        assert found == len(rec)
        rec.setflags(write=False)
        _ONE_SHOT[key] = (rec, status, chains)
    return _ONE_SHOT[key]


def stream(api, x, t, kc, sizes, arfcn, after_push=None):
    """push (x, t) in pieces of the given sizes (the rest in the last one) through a handle that follows TCH3 calls
    -> (records, status, n_chains, the records of each push)"""
    A, n = x.shape
    got, at = [], 0
    with api.RxStream(A, sps=SPS, arfcn=arfcn, tch=True, kc=kc) as s:
        for k in sizes:
            k = min(int(k), n - at)
            if at + k >= n:
                break
            got.append(s.push(x[:, at:at + k], tch=t[:, at:at + k]).copy())
            at += k
            if after_push:
                after_push(s, at)
        got.append(s.push(x[:, at:], tch=t[:, at:], last=True).copy())
        status, chains, _ = s.status()
    return np.concatenate(got), status, chains, got
