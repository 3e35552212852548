"""The error bounds of the five projection searches at each gate's flip point, without a GPU: on the ladders of
tests/margin_cases.py the array oracles, which restate the kernel's bounds operation for operation, leave unmarked
only what decides as the reference body does; every ladder does sit on its gate's threshold; and the ladders reach
from inside each bound to outside it."""
import math
import statistics

import numpy as np
import pytest

import margin_cases as M

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")
SETS = [(m, p) for m in M.MODES for p in M.PRECISIONS]
IDS = [f"{m}-{p}" for m, p in SETS]


@pytest.mark.parametrize("mode,prec", SETS, ids=IDS)
def test_every_gate_has_its_ladders(mode, prec):
    S = M.get(mode, prec)
    g = M.groups(S)
    assert set(g) == set(M.GATES[mode]) | ({"two-stage pose"} if mode == "sim3" else set())
    assert all(len(v) >= M.N_LADDERS for v in g.values())
    assert S.eps == (2.0 ** -23 if prec == "f32" else 2.0 ** -48)
    for lad in S.ladders:
        labels = [r[0] for r in lad["rungs"]]
        assert labels == sorted([-(1 << j) for j in range(M.J + 1)] + [1 << j for j in range(M.J + 1)])
        v = [r[1] for r in lad["rungs"]]
        assert all(type(x) is S.dtype for x in v) and (v == sorted(v) or v == sorted(v, reverse=True))
        mid = len(v) // 2
        assert np.nextafter(v[mid - 1], v[mid]) == v[mid]                   # rungs -1 and +1 are neighbours
        for j in range(1, M.J + 1):                                         # and rung +-2^j lies 2^j - 1 values on
            for x, y, n in ((v[mid + j], v[mid], (1 << j) - 1), (v[mid - 1 - j], v[mid - 1], (1 << j) - 1)):
                assert abs(M._ordinal(x, S.dtype) - M._ordinal(y, S.dtype)) == n
    # what the ladders vary between them: the depth over a factor of 100, the image from centre to corner, the levels
    used = {id(lad["start"]): lad["start"] for lad in S.ladders}.values()
    z = [s.z for s in used]
    assert max(z) / min(z) >= 100 and {0, 7} <= {s.L for s in used}
    assert min(abs(s.u - 620) for s in used) < 40 and max(abs(s.u - 620) + abs(s.v - 188) for s in used) > 700


def test_what_cannot_be_built_is_listed_with_its_reason():
    assert ("fkf", "depth") in M.CANNOT_BE_BUILT
    assert all(isinstance(v, str) and len(v) > 40 for v in M.CANNOT_BE_BUILT.values())
    table = {"depth": M.MODES, "bounds": M.MODES, "distance": M.MODES, "viewing": ("fuse", "scw", "local"),
             "radius": ("local",), "level": M.MODES, "window": M.MODES, "candidate": M.MODES, "chi-square": ("fuse",),
             "stereo": ("local",)}
    for gate, modes in table.items():
        for m in modes:
            assert gate in M.GATES[m] or (m, gate) in M.CANNOT_BE_BUILT, (m, gate)


@pytest.mark.parametrize("mode,prec", SETS, ids=IDS)
def test_unmarked_rungs_decide_as_the_reference_body(mode, prec):
    """Soundness, with no tolerance and no rung left out: where the array oracle leaves the status 0, its outputs are
    the reference body's on the same objects."""
    S = M.get(mode, prec)
    E = M.evaluate(S)
    unmarked = 0
    for n, (li, label, k, _) in enumerate(E["items"]):
        got = E["got"][n]
        if got[-1]:
            continue
        unmarked += 1
        base = int(E["a"]["off"][k])
        lad = S.ladders[li]
        assert M.same_as_reference(mode, got, E["ref"][n], lambda f: int(E["a"]["octave"][base + f])), (
            lad["gate"], lad["sub"], lad["start"].i, label, got, E["ref"][n])
    assert unmarked >= 2 * 0.9 * len(S.ladders)   # the outermost rungs of the closed ladders at the least


@pytest.mark.parametrize("mode,prec", SETS, ids=IDS)
def test_every_ladder_sits_on_a_flip_of_the_reference_body(mode, prec):
    """The reference body's decision at the ladder's gate differs between rungs -1 and +1, and both rungs are
    marked: two adjacent values of an input lie within any bound of each other."""
    S = M.get(mode, prec)
    E = M.evaluate(S)
    for li, lad in enumerate(S.ladders):
        r = M.ladder_rungs(S, li)
        below, above = E["dec"][r[-1]], E["dec"][r[1]]
        assert below is not None and above is not None and below != above, (lad["gate"], lad["sub"], lad["start"].i)
        assert M.marked(S, r[-1]) and M.marked(S, r[1]), (lad["gate"], lad["sub"], lad["start"].i)


@pytest.mark.parametrize("mode,prec", SETS, ids=IDS)
def test_the_ladders_span_the_bounds(mode, prec):
    """At least 90 % of the ladders of every gate are closed (their outermost rungs unmarked) at J, and a ladder
    left open is open because another decision of the reference body changes nearby.  Prints the table's row."""
    S = M.get(mode, prec)
    for gate, lads in M.groups(S).items():
        closed = [li for li in lads if M.is_closed(S, li)]
        ends = [M.mark_ends_at(S, li) for li in closed]
        print(f"| {mode} | {gate} | {prec} | {len(closed)}/{len(lads)} | {statistics.median(ends)} | {max(ends)} |")
        assert len(closed) >= 0.9 * len(lads), (gate, len(closed), len(lads))
        # the size of the bound, to a factor of two: DESIGN.md's table
        want = M.LADDER_TABLE[mode][gate][M.PRECISIONS.index(prec)]
        assert abs(statistics.median(ends) - want) <= 0.5, (gate, statistics.median(ends), want)
        for li in lads:
            if li not in closed:
                near = M.neighbour_of(S, li)
                print(f"  open: start item {S.ladders[li]['start'].i}, beside a change in {near}")
                assert near is not None, (gate, S.ladders[li]["sub"], S.ladders[li]["start"].i)


def test_j_is_the_smallest_that_leaves_no_ladder_open_for_its_own_bound():
    """J - 1 closes 90 % of every group too, but leaves ladders of the Sim3 search in float64 (two stages of
    rounding, and eps = 16 units in the last place) open with no other decision of the reference body nearby: their
    own bound reaches past 2^(J - 1) units.  At J every ladder is closed."""
    S = M.get("sim3", "f64")
    last = [li for li in range(len(S.ladders)) if M.mark_ends_at(S, li) == M.J]
    assert last and any(M.neighbour_of(S, li) is None for li in last)
    for gate, lads in M.groups(S).items():
        assert sum((M.mark_ends_at(S, li) or 99) <= M.J - 1 for li in lads) >= 0.9 * len(lads), gate


@pytest.mark.parametrize("mode,prec", SETS, ids=IDS)
def test_no_rung_for_a_device_has_its_level_quotient_on_an_integer(mode, prec):
    """The device's log need not round as NumPy's: no rung that goes to a device has |q - rint(q)| < 2^-40, so ceil(q)
    is the same under either library.  Only float64 ladders of the level gate and of the maximum distance (where q
    passes -1) have such rungs: there one unit in the last place moves q by 2^-50.  They keep their outer rungs."""
    S = M.get(mode, prec)
    E = M.evaluate(S)
    items, out = M.device_rungs(S)
    keep = [n for n in range(len(E["items"])) if n not in set(out)]
    assert len(items) == len(keep)
    for n in keep:
        q = E["quo"][n]
        assert not math.isfinite(q) or abs(q - round(q)) >= M.Q_GUARD
    # the maximum distance 1.2 mfMaxDistance is where q passes -1 (both sides clamp to level 0)
    assert all((S.ladders[E["items"][n][0]]["gate"], S.ladders[E["items"][n][0]]["sub"]) in (
        ("level", "0|1"), ("level", "inner"), ("level", "top-1|top"), ("distance", "max")) for n in out)
    if prec == "f32":
        assert not out
    else:
        left = {}
        for n in keep:
            li = E["items"][n][0]
            if S.ladders[li]["gate"] == "level":
                left.setdefault(li, []).append(abs(E["items"][n][1]))
        assert len(left) == M.N_LADDERS and all(max(v) == 1 << M.J and len(v) >= 2 for v in left.values())
