"""The host layer's carve-up of device scratch without a GPU (osmo-gmr_amd/csrc/scratch_carve.h and scratch_layouts.h
through tests/c/scratch_carve_host.cpp): the cursor itself, and every member's offset and the total of the five layouts
against the tables written down here as plain sums of rounded sizes -- never by asking the header twice.  A layout that
moved would leave every kernel correct on a GPU until two arrays met at some frame count no test runs.  (The traffic
passes' arenas are measured by the passes themselves, on the device side of the host layer: the GPU tests of the receive
loop run them.)  Once plain, once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is
preloaded)."""
import pytest

from test_chan_select_host import SAN, _build, _run

PROG = "scratch_carve_host"
COUNTS = (0, 1, 2, 31, 32, 33, 127, 128, 129, 1000)
ACQ_PEAKS = 16                                  # kAcqPeaks (gmr1_dev.h)


def up128(x):
    return (x + 127) // 128 * 128


# (member, bytes per n) in the block's order
FOLLOW3 = ([(m, 4) for m in "call p et en krv drv bt dsid dtoa frv fsid ftoa srv".split()] +
           [("feb", 104), ("seb", 212), ("cls", 1), ("need", 1), ("jeb", 416), ("jfn", 16), ("kss", 208), ("ksf", 384)] +
           [(m + v, k) for m, k in (("sfr", 20), ("scv", 8), ("fl", 10), ("fcrc", 4), ("fcv", 4)) for v in "01"])
FOLLOW9 = [("eb", 662), ("sid", 4), ("rv", 4), ("cls", 1), ("need", 1), ("src", 12), ("call", 4), ("ks", 658), ("fl2", 64),
           ("tl2", 64), ("fcrc", 4), ("fcv", 4), ("tcv", 4)]
# per carrier: (member, bytes, per candidate slot?)
ACQ = [("base", 8, 0), ("len", 8, 0), ("stat", 4, 0), ("align", 4, 0), ("base_align", 4, 0), ("ferr", 4, 0), ("can3", 4, 0),
       ("off", 8, 1), ("peaks", 4, 1), ("toa1", 4, 0), ("rv1", 4, 0), ("ftoa", 4, 0), ("fe", 4, 0), ("count", 4, 0),
       ("ctoa", 4, 1), ("cfe", 4, 1), ("snr", 4, 1), ("live", 4, 1), ("fs", 4, 1)]
AUDIO_BYTES, ACQ_REC_BYTES = 656, 216           # struct gmr1_hip_rx_audio, struct gmr1_hip_fcch_acq (gmr1_hip.h)


def sized(name, *counts):
    """the layout as [(member, bytes)] at these counts"""
    if name == "follow3":
        return [(m, k * counts[0]) for m, k in FOLLOW3]
    if name == "follow9":
        return [(m, k * counts[0]) for m, k in FOLLOW9]
    if name == "acq":
        return [(m, k * counts[0] * (counts[1] if slot else 1)) for m, k, slot in ACQ]
    if name == "audio":
        return [("slot", 4 * counts[1]), ("sink", AUDIO_BYTES * counts[0])]
    assert name == "acqblock"
    return [("offset", 8 * counts[0]), ("length", 8 * counts[0]), ("results", ACQ_REC_BYTES * counts[0])]


def restated(members):
    """[(member, offset)] and the total of [(member, bytes)]"""
    rows, at = [], 0
    for m, b in members:
        rows.append((m, at))
        at += up128(b)
    return rows, at


def printed(answer):
    w = answer.split()
    rows = [(w[i], int(w[i + 1])) for i in range(0, len(w), 2)]
    assert rows[-1][0] == "bytes"
    return rows[:-1], rows[-1][1]


def compare(answer, members, query):
    rows, total = printed(answer)
    extra = dict(r for r in rows if r[0] == "up_bytes")
    rows = [r for r in rows if r[0] != "up_bytes"]
    want_rows, want_total = restated(members)
    assert rows == want_rows, (query, rows, want_rows)
    assert total == want_total, (query, total, want_total)
    return extra


def layout_queries():
    q = [("follow3", n) for n in COUNTS] + [("follow9", n) for n in COUNTS]
    q += [("acq", n, ACQ_PEAKS) for n in (1, 2, 3, 16)]
    q += [("audio", c, n) for c in COUNTS for n in COUNTS]
    q += [("acqblock", a) for a in COUNTS]
    return q


@pytest.fixture(scope="module", params=([], SAN), ids=("plain", "asan_ubsan"))
def exe(request, tmp_path_factory):
    return _build(tmp_path_factory.mktemp("carve"), request.param, PROG)


def ask(exe, queries):
    out = _run(exe, [], "".join(" ".join(str(v) for v in q) + "\n" for q in queries)).splitlines()
    assert len(out) == len(queries)
    return out


def test_the_cursor(exe):
    assert _run(exe, ["carve"], "").strip() == "ok"


def test_every_layout_lies_where_the_tables_say(exe):
    queries = layout_queries()
    for q, answer in zip(queries, ask(exe, queries)):
        extra = compare(answer, sized(*q), q)
        if q[0] == "acqblock":
            assert extra["up_bytes"] == 2 * up128(8 * q[1])       # what goes up: offsets and lengths
    assert ask(exe, [("sizes",)])[0].split() == [str(AUDIO_BYTES), str(ACQ_REC_BYTES)]


def test_members_are_disjoint_where_every_array_is_one_line(exe):
    queries = [("follow3", 1), ("follow9", 1), ("acq", 1, ACQ_PEAKS), ("audio", 1, 1), ("acqblock", 1)]
    for q, answer in zip(queries, ask(exe, queries)):
        rows, total = printed(answer)
        spans = sorted((at, at + b) for (m, at), (_, b) in zip([r for r in rows if r[0] != "up_bytes"], sized(*q)))
        assert all(b > 0 for _, b in sized(*q))
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 <= b0, (q, spans)
        assert spans[0][0] == 0 and spans[-1][1] <= total


def test_the_comparison_sees_two_neighbours_swapped(exe):
    """the soft bits of the FACCH3 and of the speech burst, 104 and 212 bytes a frame, with each other's size: every name
    stays where it is, only the offsets behind them move"""
    q = ("follow3", 33)
    answer = ask(exe, [q])[0]
    members = sized(*q)
    compare(answer, members, q)
    i = [m for m, _ in members].index("feb")
    (a, size_a), (b, size_b) = members[i], members[i + 1]
    members[i], members[i + 1] = (a, size_b), (b, size_a)
    assert [m for m, _ in members] == [m for m, _ in sized(*q)]
    with pytest.raises(AssertionError):
        compare(answer, members, q)
