"""The one description of the layer-1 codes without a GPU (osmo-gmr_amd/csrc/l1_codes.h and nt9_map.h through
tests/c/l1_codes_host.cpp): polynomials, CRCs, the 51 puncturing masks, the puncturer, the scrambler, the interleaver
positions, the CRC unit registers and the four NT9 gather maps, against the reference's files as ref_parse reads them (or
tests/golden/ref_tables.json where they are absent) and the formulas restated here from the cited lines -- never by asking
the header twice.  Every kernel table maker, the encoder plans and the exported libgmr1-l1 objects are made from that header.
Once plain, once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import numpy as np
import pytest

import ref_parse
import test_chan_select_host as host

pytestmark = pytest.mark.skipif(not ref_parse.available(), reason="neither the reference's sources nor the golden tables")


@pytest.fixture(scope="module", params=([], host.SAN), ids=("plain", "asan_ubsan"))
def out(request, tmp_path_factory):
    """the program's lines: {section: {name: [int...]}} (sections without a name: {section: [int...]})"""
    exe = host._build(tmp_path_factory.mktemp("l1_codes"), request.param, "l1_codes_host")
    res = {}
    for ln in host._run(exe, [], "").splitlines():
        w = ln.split()
        if w[0] in ("scramble", "tch3_pos", "constexpr_mismatches"):
            res[w[0]] = [int(v) for v in w[1:]]
        elif w[0] == "crc_unit":
            res.setdefault(w[0], {})[(w[1], int(w[2]))] = [int(v) for v in w[3:]]
        else:
            res.setdefault(w[0], {})[w[1]] = [int(v) for v in w[2:]]
    return res


def scrambler(n):
    """scramb.c:39-52: b = bit 14 ^ bit 0 of the 16-bit register, shifted in at the bottom"""
    s = ref_parse.parse_scramb()
    assert s["step_bit14_xor_bit0"]
    r, bits = s["reg_init"], []
    for _ in range(n):
        b = ((r >> 14) ^ r) & 1
        r = ((r << 1) | b) & 0xFFFF
        bits.append(b)
    return bits


def intra(N, k):
    """interleave.c:46-87"""
    assert ref_parse.parse_interleave()["index_5kc_and_7"]
    return N * ((5 * k) & 7) + (k >> 3)


def test_the_constant_expressions_equal_their_run_time_twins(out):
    assert out["constexpr_mismatches"] == [0]


def test_polynomials_and_code_words_equal_conv_c(out):
    codes = ref_parse.parse_conv()
    assert sorted(out["polys"]) == sorted(codes)
    for name, c in codes.items():
        assert out["polys"][name] == c["polys_table"], name
        # reg = state << 1 | input
        assert out["words"][name] == [w for row in c["next_output"] for w in row], name


def test_crcs_equal_crc_c(out):
    crcs = ref_parse.parse_crc()
    assert sorted(out["crc"]) == sorted(crcs)
    for name, (bits, poly, init, rem) in crcs.items():
        assert out["crc"][name] == [bits, poly] and (init, rem) == (0, 0), name


def test_all_51_masks_equal_punct_c(out):
    masks = ref_parse.parse_punct()
    assert len(masks) == 51 and list(out["punct"]) == list(masks)              # punct.c's order
    for name, m in masks.items():
        assert out["punct"][name] == [m["r"], m["L"], m["N"]] + m["mask"], name


def test_scrambler_bits(out):
    assert out["scramble"] == scrambler(662)


def test_intra_positions(out):
    assert sorted(int(n) for n in out["intra"]) == [12, 14, 33, 53, 54, 80, 81]
    for n, pos in out["intra"].items():
        N = int(n)
        assert pos == [intra(N, k) for k in range(8 * N)], N
        assert sorted(pos) == list(range(8 * N))


def test_tch3_positions(out):
    """tch3.c:60-76: bits_ep[ij + 5 ii] for ii < 8, bits_ep[ij + 4 ii + 8] above, kc = 24 ij + ii"""
    want = [(kc // 24) + (5 * (kc % 24) if kc % 24 < 8 else 4 * (kc % 24) + 8) for kc in range(104)]
    assert out["tch3_pos"] == want and sorted(want) == list(range(104))


# chain: (code outputs N, unpunctured coded bits, first / main / last scheme, repeat) -- tch9.c:56-79, facch9.c:42-48,
# xch_dc12.c:45-54, tch3.c:44-50
PUNCTURED = {
    "tch9_2k4": (5, 148 * 5, "k5_15_P53", "k5_15_P23", "k5_15_Ps53", 41),
    "tch9_4k8": (3, 244 * 3, "k5_13_P15", "k5_13_P25", "k5_13_Ps15", 41),
    "tch9_9k6": (2, 484 * 2, "k5_12_P25", "k5_12_P23", "k5_12_Ps25", 158),
    "xch_dc12": (3, 208 * 3, None, "k9_13_P1213", None, 0),
    "tch3": (2, 48 * 2, None, "k5_12_P12", None, 0),
}


def punctured(chain):
    masks = ref_parse.parse_punct()
    N, cl, pre, main, post, rep = PUNCTURED[chain]
    m = lambda n: masks["gmr1_punct_" + n] if n else None
    return ref_parse.puncturer_generate(N, cl, m(pre), m(main), m(post), rep)


@pytest.mark.parametrize("chain", sorted(PUNCTURED))
def test_puncturer_equals_the_reference_generator(out, chain):
    assert out["punctured"][chain] == punctured(chain)
    assert len(punctured(chain)) == PUNCTURED[chain][1] - {"xch_dc12": 432, "tch3": 72}.get(chain, 648)


def test_facch9_punctures_nothing(out):
    assert out["punctured"]["facch9"] == []


def crc_bits(bits, poly, msgs):
    """osmo_crcXXgen_compute_bits with init 0 and no final xor, over the rows of msgs"""
    crc = np.zeros(msgs.shape[0], np.int64)
    for i in range(msgs.shape[1]):
        fb = ((crc >> (bits - 1)) & 1) ^ msgs[:, i]
        crc = ((crc << 1) & ((1 << bits) - 1)) ^ (fb * poly)
    return crc


@pytest.mark.parametrize("n", (16, 76, 123, 192, 300))
def test_crc_unit_registers(out, n):
    """crc_unit(k, n) is the CRC of the n-bit message whose only set bit is bit k"""
    for name, (bits, poly, _, _) in ref_parse.parse_crc().items():
        assert out["crc_unit"][(name, n)] == crc_bits(bits, poly, np.eye(n, dtype=np.int64)).tolist(), (name, n)


# kind: (chain of PUNCTURED or None, N, information bits, interleaver N, pad bits in front, inter-burst interleaved)
NT9 = {0: ("tch9_2k4", 5, 144, 81, 0, True), 1: ("tch9_4k8", 3, 240, 81, 0, True), 2: ("tch9_9k6", 2, 480, 81, 0, True),
       3: (None, 2, 316, 80, 4, False)}


@pytest.mark.parametrize("kind", sorted(NT9))
def test_nt9_gather_maps(out, kind):
    """Entry of coded bit ii of the (len + 4) * N unpunctured ones (tch9.c:139-203, facch9.c:106-160): bit 31 punctured; else
    the q-th sent bit sits at x = intra(q) + pad of the 648 scrambled positions; SACCH's 10 bits follow position 51 in the
    658 ciphered bits (index m, bits 11-20), the 4 status bits follow position 51 in the 662 e-bits (index e, bits 0-9);
    bit 10 the scrambler's bit x; bits 21-22 how many bursts back the bit was sent: 2 - x % 3 (gmr1_deinterleave_inter,
    N = 3, interleave.c:163-186)."""
    chain, N, length, iN, pad, inter = NT9[kind]
    cl = (length + 4) * N
    gone = set(punctured(chain)) if chain else set()
    scr = scrambler(648)
    want, q = [], 0
    for ii in range(cl):
        if ii in gone:
            want.append(0x80000000)
            continue
        x = intra(iN, q) + pad
        m = x if x < 52 else x + 10
        e = m if m < 52 else m + 4
        want.append(e | (scr[x] << 10) | (m << 11) | ((2 - x % 3 if inter else 0) << 21))
        q += 1
    assert q == 8 * iN and out["nt9_map"][str(kind)] == want
