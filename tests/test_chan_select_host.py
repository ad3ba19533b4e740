"""The resampler's launch rule without a GPU (osmo-gmr_amd/csrc/chan_select.h through tests/c/chan_select_host.cpp): period,
spans, refusal, tap bank, window, outputs per lane, waves per work-group and the grid of every plan the tests run, against
values written down here or worked out with exact fractions (chan_grid_cases.resamp_form) -- never by asking the rule.  On a
GPU a wrong choice among the forms leaves every output correct and only moves a time, and a wrong refusal shows at a plan
nobody runs.  Once plain, once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is
preloaded)."""
import os
import shutil
import subprocess
from fractions import Fraction

import pytest

import chan_grid_cases as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
FORMS = {0: "none", 1: "refused", 2: "one", 3: "two", 4: "shared"}

FILTERBANK = cg.FILTERBANK
# the direct mode at 2.0 Msps (decimation 7 x 6: 47 619 Hz into the resampler) and what else the plans' table says
DIRECT_2M = {1: "k_resamp<30,256>", 2: "k_resamp<30,128>", 3: "k_resamp2<WG=2>", 4: "k_resamp2<WG=4>", 5: "k_resamp2<WG=4>",
             8: "k_resamp2<WG=4>", 16: "k_resamp2<WG=1>"}
REFUSED = {(1.0e6, 1): 636, (1.5e6, 1): 602}             # (rate, sps): span, past the 512 samples of the 96-tap window


def _query(step, tpf, T, n_out, ext=0, stream=0, o0=0, one_only=0, shared_ring=0, wg1=0, n_slots=3):
    return (step.numerator, step.denominator, tpf, T, n_out, ext, stream, o0, one_only, shared_ring, wg1, n_slots)


def _want(q):
    num, den, tpf, T, n_out, ext, stream, o0, one_only, shared_ring, wg1, n_slots = q
    if n_slots <= 0:
        return dict(form="none")
    return cg.resamp_form(Fraction(num, den), tpf, T, n_out, ext=bool(ext), stream=bool(stream), o0=o0, planar=ext == 2,
                          one_only=bool(one_only), shared_ring=bool(shared_ring), wg1=bool(wg1))


def _cases():
    """(name, query, what is written down for it beyond the restatement)"""
    out = []
    T = 20663
    for sps, (P, Q, span, form) in FILTERBANK.items():
        st = cg.fb_step(sps)
        n_out = cg.resamp_count(st, cg.RRC_J0, T)
        out.append(("filterbank sps %d" % sps, _query(st, 30, T, n_out), dict(P=P, Q=Q, launched_span=span, form=form)))
        # the planar call of the same plan: one output per lane, EXT
        out.append(("planar sps %d" % sps, _query(st, 30, T, n_out, ext=2),
                    dict(form="k_resamp<30,%d,EXT>" % (256 if sps == 1 else 128))))
        # a streamed push of its last third
        out.append(("streamed sps %d" % sps, _query(st, 30, T, n_out, stream=1, o0=2 * n_out // 3),
                    dict(form="k_resamp<30,%d>" % (256 if sps == 1 else 128))))
    for fs in (1.0e6, 1.25e6, 1.5e6, 2.0e6, 2.5e6, 4.0e6):
        for sps in (1, 2, 3, 4, 5, 8, 16):
            d1, d2, st, tpf, nt = cg.direct_numbers(fs, sps)
            bank = 30 if tpf <= 30 else 96
            T = 200000 // d1 // d2
            extra = {}
            if fs == 2.0e6:
                extra["form"] = DIRECT_2M[sps]
            if (fs, sps) in REFUSED:
                extra.update(form="refused", span=REFUSED[(fs, sps)])
            elif bank == 96:
                extra["form"] = "k_resamp<96,512>"
            if (fs, sps) == (2.5e6, 3):
                extra.update(form="k_resamp2<WG=1>", span_r=124)
            out.append(("direct %.2f Msps sps %d" % (fs / 1e6, sps), _query(st, bank, T, cg.resamp_count(st, (nt // 2) % 32, T)), extra))
    for fs in (2.048e6, 1.92e6, 2.4e6):
        st = cg.pre_step(fs)
        for ext in (0, 1):
            out.append(("pre-resampler %.3f Msps ext %d" % (fs / 1e6, ext), _query(st, 30, 200000, 200000, ext=ext),
                        # (the rate goes up by under 2 %: 128 phases span 125 or 126 inputs + 32, past the tight window)
                        dict(form="k_resamp<30,128,EXT>" if ext else "k_resamp<30,128>")))
    big = 1 << 20
    # the limits, each from floor(63 r) + taps + 2 (floor(127 r) for two outputs per lane) at r = step / 32
    lim = [
        ("span == 256", Fraction(32 * 224, 63), 30, dict(span=256, form="k_resamp<30,256>")),
        ("span == 257", Fraction(32 * 225, 63), 30, dict(span=257, form="refused")),
        ("span == 512", Fraction(32 * 414, 63), 96, dict(span=512, form="k_resamp<96,512>")),
        ("span == 513", Fraction(32 * 415, 63), 96, dict(span=513, form="refused")),
        ("span == 128", Fraction(32 * 96, 63), 30, dict(span=128, form="k_resamp<30,128>")),
        ("span == 129", Fraction(32 * 97, 63), 30, dict(span=129, form="k_resamp<30,256>")),
        ("span_r == 128", Fraction(32 * 96, 127), 30, dict(span_r=128, form="k_resamp2<WG=1>")),
        ("span_r == 129", Fraction(32 * 97, 127), 30, dict(span_r=129, form="k_resamp<30,128>")),
        # one input per output: the rate does not go up, one output per lane; P = 1
        ("P == 1", Fraction(32), 30, dict(P=1, Q=1, form="k_resamp<30,128>", gx=1)),
        # just below: 127 outputs per 128 inputs ... and just above one input per output
        # (128 phases then span 126 inputs + 32: two outputs per lane need r <= 96 / 127 -- the rule's own test that the rate
        # goes up is implied by span_r <= 128, and so is P >= 2)
        ("rate just up", Fraction(32 * 127, 128), 30, dict(P=128, Q=127, span=94, form="k_resamp<30,128>")),
        ("rate just down", Fraction(32 * 129, 128), 30, dict(P=128, form="k_resamp<30,128>")),
        ("tpf 31", Fraction(32 * 2, 3), 31, dict(form="refused")),
        # the shortest period that takes two outputs per lane, and one of exactly one group of 128 outputs
        ("P == 2", Fraction(16), 30, dict(P=2, Q=1, span_r=95, form="k_resamp2<WG=1>", gx=1)),
        ("P == 128", Fraction(32 * 95, 128), 30, dict(P=128, Q=95, form="k_resamp2<WG=1>", gx=1)),
    ]
    for name, st, tpf, extra in lim:
        out.append((name, _query(st, tpf, big, big), extra))
    st4 = cg.fb_step(4)
    out += [
        ("T == 1", _query(st4, 30, 1, 1), dict(form="k_resamp<30,128>", gx=15)),
        ("T == 2", _query(st4, 30, 2, 6), dict(form="k_resamp2<WG=8>", gx=1, gz=1)),
        ("no output", _query(st4, 30, 0, 0), dict(form="none")),
        ("no stream", _query(st4, 30, big, big, n_slots=0), dict(form="none")),
        ("one stream", _query(st4, 30, big, big, n_slots=1), dict(form="k_resamp2<WG=8>")),
        ("one output", _query(st4, 30, 5, 1), dict(form="k_resamp2<WG=8>", gz=1)),
        # 32 periods a wave: 936 x 32 outputs are one block, one more a second
        ("gz at 32 periods", _query(st4, 30, big, 936 * 32), dict(gz=1)),
        ("gz past 32 periods", _query(st4, 30, big, 936 * 32 + 1), dict(gz=2)),
        ("stream gz at 4 periods", _query(st4, 30, big, 936 * 7, stream=1, o0=936 * 3 + 5), dict(gz=1, form="k_resamp<30,128>")),
        ("stream gz past 4 periods", _query(st4, 30, big, 936 * 7 + 1, stream=1, o0=936 * 3 + 5), dict(gz=2)),
        ("stream nothing new", _query(st4, 30, big, 5000, stream=1, o0=5000), dict(form="none")),
        ("stream one new", _query(st4, 30, big, 5001, stream=1, o0=5000), dict(form="k_resamp<30,128>", gz=1)),
        ("stream o0 < 0", _query(st4, 30, big, 5000, stream=1, o0=-1), dict(form="refused")),
        ("stream planar", _query(st4, 30, big, 5000, ext=2, stream=1), dict(form="refused")),
        ("stream rotated", _query(cg.pre_step(2.048e6), 30, big, 5000, ext=1, stream=1), dict(form="k_resamp<30,128,EXT>")),
        ("long bank rotated", _query(Fraction(32 * 1000, 117), 96, big, big, ext=1), dict(form="refused")),
        # the profiling build's switches
        ("one_only", _query(st4, 30, big, big, one_only=1), dict(form="k_resamp<30,128>", gx=15)),
        ("wg1", _query(st4, 30, big, big, wg1=1), dict(form="k_resamp2<WG=1>", gx=8)),
        # a ring per work-group: the eight waves' 1 024 phases span floor(1023 x 625 / 936) + 32 = 715 inputs, six chunks
        ("shared ring sps 4", _query(st4, 30, big, big, shared_ring=1), dict(form="k_resamp2w", nch=6, gx=1)),
        ("shared ring sps 13", _query(cg.fb_step(13), 30, big, big, shared_ring=1), dict(form="k_resamp2w", gx=3)),
        # r = 649 / 901: the 1 024 phases of eight waves start floor(1023 r) = 736 inputs apart (1024 r would say 737), + 32 =
        # 768 = six chunks exactly
        ("shared ring six chunks exactly", _query(Fraction(32 * 649, 901), 30, big, big, shared_ring=1), dict(form="k_resamp2w", nch=6, gx=1)),
        ("shared ring sps 5", _query(cg.fb_step(5), 30, big, big, shared_ring=1), dict(form="k_resamp2<WG=2>")),
        # the widest it gets: r = 765 / 1021, span_r 127, floor(1023 r) + 32 = 798 inputs, seven chunks (eight would need
        # r > 0.84, where one wave's 128 phases no longer fit the tight window)
        ("shared ring widest", _query(Fraction(32 * 765, 1021), 30, big, big, shared_ring=1), dict(form="k_resamp2w", nch=7, gx=1, span_r=127)),
    ]
    return out


def _form_name(row):
    form, P, Q, span, span_r, taps, win, per_lane, wg, nch, gx, gy, gz, runs = row
    f = FORMS[form]
    if f == "one":
        return "k_resamp<%d,%d" % (taps, win)
    if f == "two":
        return "k_resamp2<WG=%d>" % wg
    return {"shared": "k_resamp2w"}.get(f, f)


def _build(tmp_path, extra, prog="chan_select_host"):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / prog)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + extra +
                          ["-I" + os.path.join(ROOT, "osmo-gmr_amd", "csrc"), os.path.join(ROOT, "tests", "c", prog + ".cpp"),
                           "-o", exe])
    return exe


def _run(exe, args, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe] + args, input=text, capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


@pytest.mark.parametrize("extra", ([], SAN), ids=("plain", "asan_ubsan"))
def test_the_rule_on_every_plan_and_limit(tmp_path, extra):
    exe = _build(tmp_path, extra)
    cases = _cases()
    out = _run(exe, [], "".join(" ".join(str(v) for v in q) + "\n" for _, q, _ in cases))
    rows = [[int(v) for v in ln.split()] for ln in out.splitlines()]
    assert len(rows) == len(cases)
    for (name, q, extra_want), row in zip(cases, rows):
        form, P, Q, span, span_r, taps, win, per_lane, wg, nch, gx, gy, gz, runs = row
        w = _want(q)
        got_name = _form_name(row)
        ext = bool(q[5])
        if FORMS[form] == "one":
            got_name += ",EXT>" if ext else ">"
        assert got_name == w["form"], (name, got_name, w)
        if "form" in extra_want:
            assert got_name == extra_want["form"], (name, got_name, extra_want)
        if w["form"] == "none":
            assert (gx, gy, gz) == (0, 0, 0), name
            continue
        tpf = q[2]
        if tpf in (30, 96) and not (q[6] and (q[7] < 0 or q[5] == 2)):
            assert (P, Q, span, span_r, taps) == (w["P"], w["Q"], w["span"], w["span_r"], w["taps"]), (name, row, w)
            assert bool(runs) == (w["span"] <= (512 if taps == 96 else 256)), name
        got = dict(P=P, Q=Q, span=span, span_r=span_r, gx=gx, gz=gz, nch=nch,
                   launched_span=span_r if per_lane == 2 else span)
        for k, v in extra_want.items():
            if k != "form":
                assert got[k] == v, (name, k, got[k], v)
        if w["form"] == "refused":
            continue
        assert (win, per_lane, wg, gx, gy, gz) == (w["win"], w["per_lane"], w["wg"], w["gx"], q[11], w["gz"]), (name, row, w)
        assert nch == w.get("nch", 0), name
        # every output group of the period has a wave, none has two
        lanes = gx * wg * 64 * per_lane
        assert lanes >= P and (FORMS[form] == "shared" or lanes - P < 64 * per_lane), (name, lanes, P)


def test_direct_mode_search_over_the_10_khz_raster(tmp_path):
    """0.5 .. 8 Msps in steps of 10 kHz x sps 1 .. 16: the accepted plan with the widest two-outputs-per-lane window, the
    accepted plan with the widest window on the 96-tap bank, and the refused plans nearest above either window.  No plan of
    the 30-tap bank is refused anywhere on the raster (the program's "short_refused" line says so: -1), so three plans, not
    four, join the GPU grid (chan_grid_cases.DDC_SEARCH).  The steps and banks the rule is fed are the library's own
    (csrc/chan_plan.h through tests/c/chan_plan_host.cpp, which tests/test_chan_plan_host.py holds to chan_grid_cases): every
    plan it makes and every plan it refuses for its span."""
    exe = _build(tmp_path, [])
    cells = [(r * 10000.0, sps) for r in range(50, 801) for sps in range(1, 17)]
    plans = _run(_build(tmp_path, [], "chan_plan_host"), ["ddc"], "".join("%.1f %d\n" % c for c in cells)).splitlines()
    assert len(plans) == len(cells)
    lines = []
    for (fs, sps), ln in zip(cells, plans):
        head, _, text = ln.partition(" | ")
        w = head.split()
        if w[0] == "ok" or " spans " in text:
            lines.append("%d %d %s %s %s" % (int(fs), sps, w[3], w[4], w[6]))
    out = _run(exe, ["search"], "\n".join(lines) + "\n")
    print(out)
    found = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out.splitlines()}
    assert found == dict(two_widest=(1300000, 3, 126), long_widest=(920000, 1, 510), short_refused=(0, 0, -1),
                         long_refused=(620000, 1, 515))
    for key, (fs, sps) in cg.DDC_SEARCH.items():
        assert found[key][:2] == (int(fs), sps)
        d = cg.Direct(fs, sps)
        assert d.runs == (key != "long_refused")
    # the two refused plans the issue names are among the refused, and nothing at sps >= 2 is
    for (fs, sps), span in REFUSED.items():
        assert not cg.Direct(fs, sps).runs
