"""The aimed rough_multi cases (tests/fcch_multi_cases.py) on the CPU: the oracle against the float64 restatement, the
margins that make an integer comparison fair, and -- from the restatement's traces -- that every case reaches what it was
aimed at.  tests/test_gpu_fcch_multi.py then holds k_fcch_multi to the oracle on the same windows."""
import numpy as np
import pytest

import acq_cases as ac
import fcch_multi_cases as fm

CASES = fm.case_list()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def traced(pkg):
    """name -> (count, list, trace, coverage tags) of the restatement"""
    out = {}
    for c in CASES:
        cnt, toa, tr = fm.model(fm.oracle_window(pkg, c), c["sps"], c["fs"], c["N"], c["which"])
        out[c["name"]] = (cnt, toa, tr, fm.coverage(tr, cnt, c["N"]))
    return out


def test_names_are_unique_and_windows_are_valid():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        assert c["n"] >= fm.min_len(c["sps"]) and 1 <= c["N"] <= 32, c["name"]


def test_oracle_equals_the_restatement(pkg, orc, traced):
    for c in CASES:
        cnt, toa, tr, _ = traced[c["name"]]
        assert not tr.get("overread"), c["name"]         # the oracle pairs no lag with memory it has not computed
        assert fm.expected(pkg, orc, c) == (cnt, toa), (c["name"], fm.expected(pkg, orc, c), cnt, toa)
        if c["count"] is not None:
            assert cnt == c["count"], (c["name"], cnt)


def test_every_case_keeps_the_margins(traced):
    for c in CASES:
        cnt, _, tr, _ = traced[c["name"]]
        if tr.get("nLp") is None:
            assert cnt == fm.EINVAL and c["kind"] in ("zeros", "constant")       # 0 / 0: nothing is rounded
            continue
        assert not fm.margins_ok(tr), (c["name"], fm.margins_ok(tr))


def test_margins_come_from_the_measurement(pkg):
    """float32 (sums in the reference's order) against float64 over the cases: no further apart than the figures the
    margins were made of"""
    m = fm.measure(pkg, CASES)
    assert m["rel"] <= fm.REL_MEASURED and m["fpos"] <= fm.FPOS_MEASURED and m["dlp"] <= fm.DLP_MEASURED, m
    assert fm.REL_MARGIN == 50 * fm.REL_MEASURED and fm.DLP_MARGIN == 50 * fm.DLP_MEASURED
    assert fm.FPOS_MARGIN == 50 * fm.FPOS_MEASURED + 2.0 ** -11


def test_every_case_reaches_what_it_was_aimed_at(traced):
    for c in CASES:
        tags = traced[c["name"]][3]
        assert c["aims"] <= tags, (c["name"], sorted(c["aims"] - tags))


def test_coverage_of_the_whole_set(traced):
    seen = set().union(*(t[3] for t in traced.values()))
    want = {"blocked", "removed", "replaced", "gave_up", "inserted", "dropped_last", "aliased", "full", "error",
            "ends_bit31", "starts_bit0", "straddles_32", "straddles_64", "straddles_256", "straddles_2048", "last_word",
            "above_word_237", "starts_lag1", "ends_last_lag", "i0_low", "i0_high", "period", "past_end"}
    assert want <= seen, sorted(want - seen)


def test_the_list_fills_at_every_size(traced):
    for name, N in (("five_N1", 1), ("five_N2", 2), ("five_N3", 3), ("five_N32", 32), ("forty_sps1_N32", 32),
                    ("forty_sps1_N16", 16), ("forty_sps1_N2", 2)):
        c = BY_NAME[name]
        cnt, _, tr, tags = traced[name]
        assert c["N"] == N
        if name == "five_N32":
            assert cnt == 5 and "full" not in tags       # the one size five trains cannot fill
        else:
            assert cnt == N and "full" in tags, (name, cnt)
    ev = traced["five_N3"][2]["events"]
    assert sum(e["dropped_last"] for e in ev) == 2
    assert sum(e["gave_up"] for e in traced["five_N1"][2]["events"]) == 3
    for name, hits in (("forty_sps1_N32", 8), ("forty_sps1_N16", 24), ("forty_sps1_N2", 38)):
        ev = traced[name][2]["events"]
        assert sum(e["gave_up"] or e["dropped_last"] for e in ev) == hits, name


def test_what_the_aimed_cases_pin(traced):
    # trains 7488 / 4 symbols apart are one train to _peak_record at 4 samples a symbol, and two at 1
    assert traced["forty_sps4_N32"][0] < 32 == traced["forty_sps1_N32"][0]
    for name in ("alias_weak_first", "alias_strong_first"):
        assert traced[name][0] == 2 and [t // 4 for t in sorted(traced[name][1])] != [1000, 2872, 5000]
    # the periods measured
    assert [traced["period_%d" % p][2]["nLp"] for p in (7485, 7491, 7498)] == [7485, 7491, 7497]
    # the strongest lag at either end of its range
    assert traced["lag3"][2]["i0"] == 3 and traced["bounds_ends"][2]["i0"] == 1
    assert [traced["min_len_%d" % k][2]["i0"] for k in (100, 112, 116)] == [7588, 7600, 7604]
    assert traced["min_len_116"][2]["nlags"] == 15094
    # runs where they were aimed
    assert (2046, 2048) in traced["bounds_2048"][2]["runs"] and (4094, 4096) in traced["bounds_2048"][2]["runs"]
    assert traced["bounds_ends"][2]["runs"][0][0] == 1
    assert traced["bounds_last_lag"][2]["runs"][-1][1] == 7603
    assert any(a // 32 != b // 32 and a // 32 >= 244 for a, b in traced["fcch3_word_245"][2]["runs"])
    # three separate peaks survive in every FCCH3 case
    for name in ("fcch3_650ms", "fcch3_long", "fcch3_word_245"):
        cnt, toa, _, _ = traced[name]
        assert cnt >= 3 and min(np.diff(sorted(toa))) > 936, (name, toa)


def test_fcch3_650ms_window_needs_no_lag_past_the_sweep(pkg, traced):
    """The 650 ms FCCH3 window goes to the oracle with zeros behind it (acq_cases.multi_window) and to the kernel as it
    is, where lags past the sweep count as 0: the restatement gives the same list, within the margins, either way."""
    c = BY_NAME["fcch3_650ms"]
    cnt, toa, tr = fm.model(fm.window(pkg, c), c["sps"], c["fs"], c["N"], c["which"])
    assert (cnt, toa) == traced[c["name"]][:2] and not fm.margins_ok(tr)
    assert tr["past_end"] > 64 and fm.oracle_window(pkg, c).size > fm.window(pkg, c).size


def test_each_slip_of_the_kernel_is_noticed(pkg, traced):
    """What k_fcch_multi would return with one of five slips in it (fm.slipped, a replay of the traces the kernel's way):
    at least one case changes its answer for each, the aimed ones among them."""
    aimed = dict(no_before={"bounds_word", "bounds_2048", "fcch3_word_245"}, short_word={"bounds_ends", "bounds_last_lag"},
                 q_lt_n={"five_N32"}, mod_not_shifted={"forty_sps4_N32"},
                 mod_in_symbols={"alias_weak_first", "alias_strong_first", "forty_sps4_N32"})
    for c in CASES:                                      # the replay without a slip is the restatement's own answer
        cnt, toa, tr, _ = traced[c["name"]]
        assert fm.slipped(cnt, tr, c["sps"], c["N"], c["which"], None) == (cnt, toa), c["name"]
    for mut in fm.MUTATIONS:
        hit = set()
        for c in CASES:
            cnt, toa, tr, _ = traced[c["name"]]
            if fm.slipped(cnt, tr, c["sps"], c["N"], c["which"], mut) != (cnt, toa):
                hit.add(c["name"])
        assert aimed[mut] <= hit, (mut, sorted(hit))


def test_acquisition_carriers_keep_their_margins(pkg, orc):
    """The two carriers tests/test_gpu_fcch_multi.py gives the batched acquisition: the oracle's chain keeps
    acq_cases.MARGIN at every survivor decision, step 3's window keeps this module's margins, `crowded` fills the list of
    sixteen and `aliased` loses a train to the other's alias."""
    for name, x, start in fm.acq_carriers(pkg):
        rec, margins = ac.expected(orc, x, ac.SPS, start)
        assert rec["status"] == 0 and all(min(m) >= ac.MARGIN for m in margins), (name, margins)
        base, wl3 = rec["base_align"], ac.windows(ac.SPS)[1]
        cnt, _, tr = fm.model(x[base:base + wl3], ac.SPS, float(-rec["freq_err"]), ac.MAX_CHAINS)
        tags = fm.coverage(tr, cnt, ac.MAX_CHAINS)
        assert cnt == rec["n_cand"] and not fm.margins_ok(tr), (name, cnt, fm.margins_ok(tr))
        if name == "crowded":
            assert cnt == ac.MAX_CHAINS and {"full", "dropped_last"} <= tags and rec["n_chains"] == ac.MAX_CHAINS
        else:
            assert cnt == 2 and "aliased" in tags and rec["n_chains"] == 2
