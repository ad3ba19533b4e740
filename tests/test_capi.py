"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol the
headers declare, carries the same burst tables as the oracle, and refuses to compute
without a GPU (no CPU fallback)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# declared in include/ for the application's sake but defined BY the application, as in the reference
# (src/Makefile.am:8 compiles src/gsmtap.c into gmr1_rx: it allocates a libosmocore msgb, which this library does not link)
PROGRAM_SUPPLIED = {"gmr1_gsmtap_makemsg"}


def _declared_symbols():
    funcs, data = set(), set()
    for h in glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True):
        txt = open(h).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        txt = re.sub(r"//[^\n]*", "", txt)
        funcs |= set(re.findall(r"\b(gmr1_[a-z0-9_]+)\s*\(", txt))
        data |= set(re.findall(r"extern\s+(?:const\s+)?struct\s+\w+\s+(gmr1_\w+)\s*;", txt))
    return funcs, data


def _declared_prototypes():
    """name -> (return type, [parameter declarations]) of every function the headers declare"""
    protos = {}
    for h in glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True):
        txt = open(h).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        txt = re.sub(r"//[^\n]*", "", txt)
        txt = re.sub(r"(?m)^\s*#.*$", "", txt)
        for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(gmr1_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
            ret, name, params = (" ".join(x.split()) for x in m.groups())
            protos[name] = (ret, [] if params == "void" else [q.strip() for q in params.split(",")])
    return protos


# C class of a parameter or return value -> the type its row of api.SIGNATURES must carry.  Beyond the scalar classes:
# an enum is an int in this ABI, a function returning `const char *` hands back a C string, and void returns nothing.
_TABLE_TYPE = {"int": C.c_int, "int32_t": C.c_int, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
               "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "void": None}


def _table_type(decl, is_return=False):
    decl = decl.replace("const ", "").strip()
    if "*" in decl or "[" in decl:
        return C.c_char_p if is_return and decl.startswith("char") else C.c_void_p
    if not is_return:
        decl = re.sub(r"\s*\w+$", "", decl)          # drop the parameter's name
    return C.c_int if decl.startswith("enum ") else _TABLE_TYPE[decl]


def test_signature_table_matches_the_headers(pkg):
    """Every row of api.SIGNATURES against the declaration it mirrors: as many parameters, each of the type its C class
    asks for, and the same return type.  (The set of names is test_library_exports_every_declared_symbol's.)"""
    protos = _declared_prototypes()
    funcs, _ = _declared_symbols()
    assert set(protos) == funcs                        # the parser saw every declaration the name search sees
    wrong = []
    for name, (ret, params) in sorted(protos.items()):
        if name in PROGRAM_SUPPLIED:
            continue
        want = (_table_type(ret, True), *[_table_type(q) for q in params])
        if tuple(pkg.api.SIGNATURES[name]) != want:
            wrong.append((name, ret, params))
    assert not wrong, wrong


def test_typed_prototypes_leave_the_shared_handle_alone(pkg):
    """api._fn() makes function objects of its own: what load() returns keeps ctypes' defaults for raw callers."""
    lib = pkg.api.load()
    f = pkg.api._fn("gmr1_hip_burst_info")
    assert f is pkg.api._fn("gmr1_hip_burst_info") and f is not lib.gmr1_hip_burst_info
    assert tuple(f.argtypes) == (C.c_int, C.c_void_p) and f.restype is C.c_int
    for name in pkg.api.EXPORTED_FUNCTIONS:
        assert getattr(lib, name).argtypes is None, name


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.api.load()
    funcs, data = _declared_symbols()
    assert funcs and data
    assert PROGRAM_SUPPLIED <= funcs
    funcs -= PROGRAM_SUPPLIED
    for name in sorted(funcs | data):
        assert hasattr(lib, name), f"{name} is declared in include/ but not exported"
    # and the python mirror lists the same set
    assert set(pkg.api.EXPORTED_FUNCTIONS) == funcs
    assert set(pkg.api.EXPORTED_DATA) == data


def test_version_and_error_strings(pkg):
    lib = pkg.api.load()
    assert b"gfx950" in lib.gmr1_hip_version()
    assert isinstance(lib.gmr1_hip_last_error(), bytes)


def test_burst_tables_equal_oracle_tables(pkg, orc):
    """Two independent transcriptions of ETSI TS 101 376-5-2 7.4 (reference src/sdr/nb.c)."""
    for name in pkg.api.BURST_IDS:
        assert pkg.api.burst_format(name) == orc.burst_format(name), name
    with pytest.raises(pkg.api.Gmr1HipError):
        pkg.api.burst_info(99)


def test_burst_table_invariants(pkg):
    for name in pkg.api.BURST_IDS:
        f = pkg.api.burst_format(name)
        used = np.zeros(f.length, int)
        for p, l in f.data:
            used[p:p + l] += 1
        assert sum(l for _, l in f.data) * f.nbits == f.ebits
        for seq in f.sync:
            u = used.copy()
            for p, syms in seq:
                u[p:p + len(syms)] += 1
                assert max(syms) < (1 << f.nbits) * (2 if f.nbits == 1 else 1)
            assert u.max() == 1, name                     # sync and data never overlap
            assert u[:2].sum() == 0 and u[-3:].sum() == 0  # guard symbols stay empty


def test_exported_struct_layout_matches_reference_abi(pkg):
    """gmr1_bcch_burst etc. are pointer-linked structs laid out like the reference's
    (include/osmocom/gmr1/sdr/pi4cxpsk.h:43-98); walk one through raw memory."""
    lib = pkg.api.load()

    class Mod(C.Structure):
        _fields_ = [("rotation", C.c_float), ("nbits", C.c_int), ("syms", C.c_void_p), ("bits", C.c_void_p)]

    class Sync(C.Structure):
        _fields_ = [("pos", C.c_int), ("len", C.c_int), ("syms", C.c_uint8 * 32), ("_ref", C.c_void_p)]

    class Data(C.Structure):
        _fields_ = [("pos", C.c_int), ("len", C.c_int)]

    class Burst(C.Structure):
        _fields_ = [("mod", C.POINTER(Mod)), ("guard_pre", C.c_int), ("guard_post", C.c_int),
                    ("len", C.c_int), ("ebits", C.c_int), ("sync", C.POINTER(Sync) * 4),
                    ("data", C.POINTER(Data))]

    b = Burst.in_dll(lib, "gmr1_dc6_burst")
    assert (b.guard_pre, b.guard_post, b.len, b.ebits) == (2, 3, 234, 432)
    assert abs(b.mod.contents.rotation - np.pi / 4) < 1e-6 and b.mod.contents.nbits == 2
    assert (b.sync[0][0].pos, b.sync[0][0].len, list(b.sync[0][0].syms[:7])) == (28, 7, [0, 0, 0, 2, 2, 0, 2])
    assert b.sync[0][3].pos == -1 and not b.sync[1]
    assert (b.data[1].pos, b.data[1].len) == (35, 84) and b.data[4].pos == -1
    sd = Burst.in_dll(lib, "gmr1_sdcch_burst")
    assert all(bool(sd.sync[i]) for i in range(4))       # 4 sequences, no NULL terminator


# every gmr1_* function / data object the reference's application references (src/gmr1_rx.c), except
# gmr1_gsmtap_makemsg, which is compiled into the program itself from src/gsmtap.c (src/Makefile.am:8)
GMR1_RX_LINKS = [
    "gmr1_a5", "gmr1_bcch_burst", "gmr1_bcch_decode", "gmr1_ccch_decode", "gmr1_dc6_burst", "gmr1_dkab_demod",
    "gmr1_facch3_decode", "gmr1_facch9_decode", "gmr1_fcch_burst", "gmr1_fcch_fine", "gmr1_fcch_rough",
    "gmr1_fcch_rough_multi", "gmr1_fcch_snr", "gmr1_interleaver_init", "gmr1_nt3_facch_burst",
    "gmr1_nt3_speech_burst", "gmr1_nt9_burst", "gmr1_pi4cxpsk_demod", "gmr1_pi4cxpsk_detect", "gmr1_tch3_decode",
    "gmr1_tch9_decode",
]


def test_library_covers_what_gmr1_rx_links_against(pkg):
    lib = pkg.api.load()
    for name in GMR1_RX_LINKS:
        assert hasattr(lib, name), f"gmr1_rx.c needs {name}"
    # the list above is what the file references (read from it, or from tests/golden/ref_tables.json where it is absent)
    import ref_parse
    used = set(ref_parse.parse_gmr1_rx_identifiers())
    used -= {"gmr1_gsmtap_makemsg", "gmr1_interleaver", "gmr1_pi4cxpsk_burst"}     # own code / type names
    assert used == set(GMR1_RX_LINKS)


_c64 = lambda n: np.zeros(n, np.complex64)
_u8 = lambda *shape: np.zeros(shape, np.uint8)
_i8 = lambda *shape: np.zeros(shape, np.int8)
_NULL_HANDLE = dict(_handle=C.c_void_p(), _n_sel=1)

# what each call gives without a GPU, recorded from api.py as it was before its calls went through typed prototypes
_NO_GPU_RAISES = {
    -19: [
        lambda a: a.init(0),
        lambda a: a.clock_probe_dev(0),
        lambda a: a.demod_batch("bcch", _c64(1016), [0], 1016),
        lambda a: a.demod_batch("bcch", _c64(1016), [0], 1016, freq_shift=[0.0], want_ssyms=False),
        lambda a: a.demod_taps("bcch", _c64(1016)),
        lambda a: a.ccch_decode_batch(_i8(1, 432)),
        lambda a: a.rx_bcch_ccch_batch(_c64(1016), [0], [0], freq_shift=[0.0], want_ebits=False, want_ssyms=False),
        lambda a: a.fcch_rough_batch(_c64(2048), [0], 2048),
        lambda a: a.fcch_fine_batch(_c64(2048), [0], freq_shift=[0.0]),
        lambda a: a.fcch_snr_batch(_c64(2048), [0]),
        lambda a: a.fcch_rough_multi_batch(_c64(2048), [0], 2048),
        lambda a: a.facch3_decode_batch(_i8(1, 416)),
        lambda a: a.facch3_decode_batch(_i8(1, 416), ciph=_u8(1, 384)),
        lambda a: a.tch3_decode_batch(_i8(1, 212), ciph=_u8(1, 208)),
        lambda a: a.tch3_rx_batch(_c64(474), [0], 474, freq_shift=[0.0], ciph=_u8(1, 208), want_ebits=False),
        lambda a: a.detect_batch(["nt3_speech", "nt3_facch"], _c64(474), [0], 474),
        lambda a: a.detect_batch([4, 5], _c64(474), [0], 474, freq_shift=[0.0], e_toa=1.0),
        lambda a: a.mod_order_batch(_c64(474), [0], 474),
        lambda a: a.rx_run(_c64(4096), [0], [4096], max_records=4),
        lambda a: a.rx_run(_c64(4096), [0], [4096], arfcn=[7], max_records=4),
        lambda a: a.rx_run_tch(_c64(4096), _c64(4096), [0], [4096], kc=_u8(8), max_records=4),
        lambda a: a.rx_run_tch(_c64(4096), None, [0], [4096], max_records=4),
        lambda a: a.rx_run_full(_c64(4096), _c64(4096), None, [0], [4096], kc=_u8(8), max_records=4, max_big=4),
        lambda a: a.dkab_demod_batch(_c64(474), [0], 474, 0, freq_shift=0.0),
        lambda a: a.dkab_demod(_c64(474)),
        lambda a: a.a5_batch(1, _u8(8), 0, 208),
        lambda a: a.a5_batch(1, _u8(8), 0, 208, want_ul=True),
        lambda a: a.channelize_plan(2e6, 4, 4096),
        lambda a: a.channelize(_c64(4096), 2e6, [0]),
        lambda a: a.ddc_plan(2e6, 4, 4096),
        lambda a: a.ddc(_c64(4096), 2e6, [0.0]),
        lambda a: a.facch9_decode_batch(_i8(1, 662), ciph=_u8(1, 658)),
        lambda a: a.facch9_decode(_i8(662)),
        lambda a: a.rach_decode(_i8(494), 0),
        lambda a: a.tch9_decode_batch(_i8(3, 662), 0, 3),
        lambda a: a.ccch_encode_batch(_u8(1, 24)),
        lambda a: a.xch_dc12_encode_batch(_u8(1, 24)),
        lambda a: a.facch3_encode_batch(_u8(1, 10), _u8(1, 32)),
        lambda a: a.tch3_encode_batch(_u8(1, 2, 10), _u8(1, 4), ciph=_u8(1, 208)),
        lambda a: a.facch9_encode_batch(_u8(1, 38), _u8(1, 10), _u8(1, 4)),
        lambda a: a.rach_encode_batch(_u8(1, 18), [0]),
        lambda a: a.encode_single("xch_dc12", _u8(24)),
        lambda a: a.codec_decode_batch(_u8(1, 1, 10)),
        lambda a: a.codec_init_dev(0, 1, 0),
        lambda a: a.codec_decode_batch_dev(0, 1, 1, 0, 0, 0, 0),
        lambda a: a.ChanStream(2e6, [0]),
        lambda a: a.ChanStream.direct(2e6, [0.0]),
        lambda a: a.RxStream(1),
        lambda a: a.RxStream(1, arfcn=[7]),
        lambda a: a.ChanStream(None, None, **_NULL_HANDLE).out_len(16),
        lambda a: a.ChanStream(None, None, **_NULL_HANDLE).push(_c64(16)),
        lambda a: a.ChanStream(None, None, **_NULL_HANDLE).push_dev(0, 0, 16, 0, 16),
    ],
    # the _dev entries, given null addresses: refused as invalid arguments before anything is touched
    -22: [
        lambda a: a.rx_bcch_ccch_batch_dev(0, 1, 4, *[0] * 12),
        lambda a: a.rx_bcch_ccch_batch_planar_dev(0, 1, 4, 0, 1024, *[None] * 11),
        lambda a: a.iq_to_planar_dev(0, 4, 1024, 0, 0, 256),
        lambda a: a.fcch_rough_batch_dev(0, "fcch", 1, 4, 2048, 0, 0, 0, 0, 0),
        lambda a: a.rx_run_dev(0, 0, [0], [4096], max_records=4),
        lambda a: a.rx_run_dev(0, 0, [0], [4096], arfcn=[7], out=np.zeros(4, a.RX_RECORD)),
        lambda a: a.rx_run_dev_prepared(0, 0, [0], [4096], np.zeros(4, a.RX_RECORD))(),
        lambda a: a.rx_run_dev_raw(0, 0, [0], [4096], 0, 0),
        lambda a: a.ddc_dev(0, 0, 4096, 2e6, [0.0], 0, 4096),
        lambda a: a.channelize_dev(0, 0, 4096, 2e6, [0], 0, 4096),
        lambda a: a.channelize_planar_dev(0, 0, 4096, 2e6, [0], 0, 4096, 1024),
    ],
}
_NO_GPU_RETURNS = {
    -19: [
        lambda a: a.pi4cxpsk_demod("bcch", _c64(1016))["rv"],
        lambda a: a.pi4cxpsk_demod(a.CallerBurst("dc6"), _c64(976))["rv"],
        lambda a: a.ccch_decode(_i8(432))[1],
        lambda a: a.fcch_rough(_c64(2048))[0],
        lambda a: a.fcch_rough_multi(_c64(2048))[0],
        lambda a: a.facch3_decode(_i8(416))[2],
        lambda a: a.pi4cxpsk_detect(["nt3_speech", a.CallerBurst("nt3_facch")], 0.0, _c64(474))["rv"],
        lambda a: a.pi4cxpsk_mod_order(_c64(474)),
    ],
    -22: [lambda a: a.fcch_fine(_c64(2048))[0], lambda a: a.fcch_snr(_c64(2048))[0]],
}
_NO_GPU_ENCODE_SINGLE = [
    ("ccch", (_u8(24),)), ("facch3", (_u8(10), _u8(32), None)), ("tch3", (_u8(10), _u8(10), _u8(4), None, 0)),
    ("facch9", (_u8(38), _u8(10), _u8(4), None)), ("rach", (_u8(18), 0)),
]


def test_no_cpu_fallback(pkg):
    """Without a usable GPU every compute entry point fails loudly (-ENODEV)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    eb = np.zeros((4, 424), np.int8)
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.bcch_decode_batch(eb)
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.rx_bcch_ccch_batch(np.zeros(2048, np.complex64), [0], [0])
    l2, rv, _ = pkg.api.bcch_decode(eb[0])
    assert rv == -19
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.Shard(bytes(128), 0, 1)
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.xch_dc12_decode_batch(np.zeros((2, 432), np.int8))
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.tch3_rx_batch(np.zeros(1024, np.complex64), [0, 480], 474)
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.rach_decode_batch(np.zeros((2, 494), np.int8), 0)
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.xch_dc12_decode(np.zeros(432, np.int8))
    # transmit direction: encoders and modulator
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.bcch_encode_batch(np.zeros((2, 24), np.uint8))
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.tch9_encode_batch(np.zeros((3, 18), np.uint8), 0, 3, np.zeros((3, 10), np.uint8), np.zeros((3, 4), np.uint8))
    with pytest.raises(pkg.api.Gmr1HipError, match="-19"):
        pkg.api.mod_batch("bcch", np.zeros((1, 424), np.uint8))
    with pytest.raises(pkg.api.Gmr1HipError):
        pkg.api.encode_single("bcch", np.zeros(24, np.uint8))          # void call: bits_e untouched, error recorded
    rc, _ = pkg.api.pi4cxpsk_mod("bcch", np.zeros(424, np.uint8))
    assert rc == -19
    # ... and so does every other wrapper and handle class of api.py, at the smallest input its own checks accept: what
    # comes back is what the library answers (-ENODEV; -EINVAL for the null addresses the _dev entries are given here, which
    # they refuse before anything else), never a ctypes.ArgumentError or TypeError from the marshalling
    api = pkg.api
    for code, calls in _NO_GPU_RAISES.items():
        for i, call in enumerate(calls):
            with pytest.raises(api.Gmr1HipError, match=" failed with %d: " % code):
                call(api)
                pytest.fail("no error from call %d of _NO_GPU_RAISES[%d]" % (i, code))
    for code, calls in _NO_GPU_RETURNS.items():
        assert [call(api) for call in calls] == [code] * len(calls)
    for chain, args in _NO_GPU_ENCODE_SINGLE:
        with pytest.raises(api.Gmr1HipError, match="gmr1_%s_encode: no HIP device" % chain):
            api.encode_single(chain, *args)
    # the reference's void calls have no code to return: the outputs keep their fill, the error is recorded
    for out in (*api.a5(1, _u8(8), 0, 8), api.scramble_sbit(_i8(8)), api.scramble_ubit(_u8(8)), api.interleave_intra(_u8(8), 1),
                api.interleave_intra(_u8(8), 1, inverse=True), api.InterBurstInterleaver().interleave(_u8(648)),
                api.InterBurstInterleaver().deinterleave(_u8(648))):
        assert len(set(out.tolist())) == 1 and out[0] in (0xEE, 77)
    assert [int(v) for v in api.tch3_decode(_i8(212))[3:]] == [0, 0]
    l2, sa, stt, conv = api.Tch9Channel(0).decode(_i8(662))
    assert not l2.any() and conv == 0
    with pytest.raises(api.Gmr1HipError, match="gmr1_tch9_encode: no HIP device"):
        api.Tch9Encoder(0).encode(_u8(18), _u8(10), _u8(4))
    assert b"no HIP device" in api.load().gmr1_hip_last_error()
    assert sorted(api.rx_run_last_timing()) == ["acquisition_ms", "chain_ms", "handback_ms", "host_ms", "traffic_passes_ms"]
    # the handle classes: the interleaver objects are host memory (made above); the rest refuse at creation
    for cls in (api.ChanStream, api.RxStream, api.Tch9Channel, api.Tch9Encoder, api.InterBurstInterleaver, api.Codec, api.Shard):
        assert all(callable(getattr(cls, m)) for m in ("close", "__enter__", "__exit__", "__del__")), cls
    with api.Tch9Channel(0) as ch:
        assert ch.il.bits_cpp
    assert not ch.il.bits_cpp
    ch.close()                                        # a second close is a no-op
    with pytest.raises(api.Gmr1HipError, match="gmr1_codec_alloc returned NULL: no HIP device"):
        api.Codec()


def test_product_does_not_reference_oracle():
    """Nothing under the package or include/ may import, include or link the oracle."""
    bad = []
    for d in ("osmo-gmr_amd", "include"):
        for path in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True):
            if os.path.isfile(path) and path.endswith((".py", ".h", ".hip", ".cpp", ".c", ".inc")):
                txt = open(path, errors="replace").read()
                if re.search(r"oracle_lib|liborc|import\s+orc_chan|from\s+orc_chan|orc_[a-z0-9_]+\(|#include\s+\"orc_", txt):
                    bad.append(path)
    assert not bad, bad


def test_gsmtap_packet_layout(pkg):
    """gmr1_gsmtap_makemsg (reference src/gsmtap.c:43-71): version 2, 4-word header, type GMR1_UM,
    frame number big-endian, sub_type = channel type, L2 appended.  Host-only, no GPU needed."""
    api = pkg.api
    rec = np.zeros(1, api.RX_RECORD)
    rec["arfcn"], rec["type"], rec["fn"], rec["tn"], rec["len"] = 1007, 2, 0x00A1B2C3, 17, 24
    rec["l2"][0] = np.arange(24, dtype=np.uint8) + 100
    pkt = api.gsmtap_pack(rec[0])
    assert len(pkt) == 40
    assert pkt[:4] == bytes([2, 4, 0x0A, 17]) and pkt[4:8] == bytes(4)
    assert pkt[8:12] == bytes([0x00, 0xA1, 0xB2, 0xC3]) and pkt[12] == 2 and pkt[13:16] == bytes(3)
    assert pkt[16:] == bytes(range(100, 124))
    pkt2 = api.gsmtap_pack(rec[0], with_arfcn=True)
    assert pkt2[4:6] == bytes([1007 >> 8, 1007 & 0xFF]) and pkt2[6:] == pkt[6:]


def test_gsmtap_big_packet_layout(pkg):
    api = pkg.api
    rec = np.zeros(1, api.RX_BIG_RECORD)
    rec["type"], rec["fn"], rec["tn"], rec["len"] = 0x18, 123456, 5, 60
    rec["l2"][0][:60] = np.arange(60, dtype=np.uint8)
    pkt = api.gsmtap_pack_big(rec[0])
    assert len(pkt) == 76 and pkt[:4] == bytes([2, 4, 0x0A, 5]) and pkt[12] == 0x18
    assert pkt[8:12] == (123456).to_bytes(4, "big") and pkt[16:] == bytes(range(60))


def test_headers_are_plain_c_and_link(pkg, tmp_path):
    """tests/c/abi_smoke.c: a C99 program over every public header, linked against the library, run without a GPU."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = os.path.join(ROOT, "tests", "c", "abi_smoke.c")
    exe = str(tmp_path / "abi_smoke")
    libdir = os.path.dirname(pkg.api.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + libdir, "-lgmr1_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip()


def test_exported_code_descriptions_agree_with_the_oracle(pkg, orc):
    """l1/conv.h + l1/punct.h objects and gmr1_puncturer_generate (host code) without the reference tree: the TCH9 9k6
    code specialised as tch9.c:73-78 does has the oracle's trellis and the 320 punctured positions of the fixture."""
    import json
    lib = pkg.api.load()

    class ConvCode(C.Structure):
        _fields_ = [("N", C.c_int), ("K", C.c_int), ("len", C.c_int), ("term", C.c_int),
                    ("next_output", C.POINTER(C.c_uint8 * 2)), ("next_state", C.POINTER(C.c_uint8 * 2)),
                    ("next_term_output", C.c_void_p), ("next_term_state", C.c_void_p), ("puncture", C.POINTER(C.c_int))]
    code = ConvCode()
    C.memmove(C.byref(code), C.addressof(ConvCode.in_dll(lib, "gmr1_conv_k5_12")), C.sizeof(ConvCode))
    code.len = 480
    addr = lambda n: C.c_void_p(C.addressof(C.c_int.in_dll(lib, n)))
    lib.gmr1_puncturer_generate.restype = C.c_int
    rc = lib.gmr1_puncturer_generate(C.byref(code), addr("gmr1_punct_k5_12_P25"), addr("gmr1_punct_k5_12_P23"),
                                     addr("gmr1_punct_k5_12_Ps25"), C.c_int(158))
    assert rc == 0
    got = []
    while code.puncture[len(got)] >= 0:
        got.append(code.puncture[len(got)])
    with open(os.path.join(ROOT, "tests", "golden", "known_answers.json")) as f:
        assert got == json.load(f)["tch9_9k6_punctured"]
    assert got == list(orc.tch9_punct(2))
    C.CDLL(None).free(code.puncture)
    for s in range(16):
        assert [code.next_state[s][0], code.next_state[s][1]] == [(2 * s) & 15, (2 * s + 1) & 15]
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "known_answers.json")))["conv_spot"]["k5_12"]
    for s, row in g["next_output_rows"].items():
        assert [code.next_output[int(s)][0], code.next_output[int(s)][1]] == row


def test_plain_makefile_recipe(tmp_path):
    """The repository's Makefile (what a C maintainer runs instead of build.py; reference src/Makefile.am:1-24,
    src/sdr/Makefile.am:5-7, src/l1/Makefile.am:5-9): a dry run of `make all check install` names hipcc for every source build.py
    compiles, the pkg-config file comes out right, and `make install` of an (already built) library lays out lib/, include/ and
    lib/pkgconfig/ under DESTDIR.  (The compile itself is __graft_entry__.build()'s: the same commands.)"""
    import shutil
    import subprocess
    if shutil.which("make") is None:
        pytest.skip("no make")
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.build.build()                      # (a no-op when the library is up to date)
    r = subprocess.run(["make", "-n", "-B", "all", "check"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for src in pkg.build.HIP_SOURCES + pkg.build.CXX_SOURCES:
        assert f"osmo-gmr_amd/csrc/{src}" in r.stdout, src
    assert "--offload-arch=gfx950" in r.stdout and "-shared" in r.stdout and "abi_smoke" in r.stdout
    bdir = str(tmp_path / "b")
    r = subprocess.run(["make", f"BUILD={bdir}", f"{bdir}/gmr1_hip.pc", "PREFIX=/opt/gmr1"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pc = open(os.path.join(bdir, "gmr1_hip.pc")).read()
    assert "prefix=/opt/gmr1" in pc and "Libs: -L${libdir} -lgmr1_hip" in pc and "Cflags: -I${includedir}" in pc
    # install: the library is there already (build()), so only the copy runs -- never a compile (-o: the objects are not remade)
    dest = str(tmp_path / "dest")
    r = subprocess.run(["make", "-o", pkg.build.LIB.replace(ROOT + "/", ""), f"BUILD={bdir}", "install", "PREFIX=/usr", f"DESTDIR={dest}"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(os.path.join(dest, "usr/lib/libgmr1_hip.so"))
    assert os.path.exists(os.path.join(dest, "usr/lib/pkgconfig/gmr1_hip.pc"))
    assert os.path.exists(os.path.join(dest, "usr/include/gmr1_hip.h"))
    assert os.path.exists(os.path.join(dest, "usr/include/osmocom/gmr1/sdr/pi4cxpsk.h"))
