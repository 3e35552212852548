"""Cases for k_local_search on the geometry of tests/fuse_cases.py (identity pose, fx = fy = 64, cx = cy = 0, bf = 32,
the image [0, 640] x [0, 480], 16 px cells, four levels with the scale factors 1, 1.25, 1.5, 2): a point made by
`pt(u, v)` lies at depth 1, lands on exactly (u, v) with ur = u - 32, looks straight at the camera (its viewing cosine
is 1 up to rounding, so its radius is 2.5 scale[level]) and every gate is decided by small dyadic numbers.  `axis(c)`
makes the point (0.75, 0, 1), which is 1.25 away and projects to (48, 0), with the normal (0, 0, c): its viewing cosine
is exactly c / 1.25, and at v = 0 every summed term of v is zero, so the bound on v is zero too and the image bound
marks nothing.  The viewing cosine's limit is 0.5 and th is 1 with the flag off unless a case says otherwise.

A search is a target frame, a limit and a list of rows of one shared point table; a frame has one blocked byte and one
right coordinate per feature.  Each case carries its claim as a `check` over the array oracle's results (a dict by
output name), which tests/test_local_search_cpu.py runs, so the GPU test that compares the kernel with the oracle cannot
pass on inputs that miss the situation.

A case: name, frames (fuse_oracle keyframe dicts), blocked (per frame, or None), pt_f64 / pt_desc (the point table),
limits / srch_kf / items (per search its limit, its target and its rows of the table), th, th_on, eps, check(out) and
marked (the items built to come back ORBFE_FUSE_MARGINAL; no other item may).

Also the stand-ins with the surface Tracking.search_local_points reads, and the drivers of the golden
tests/golden/local_search.npz, shared by its generator and the tests.
"""
from __future__ import annotations

import math

import numpy as np

import fkf_cases as KC
import fuse_cases as FC
import fuse_oracle as O
import local_search_oracle as LO
import matcher_world as MW
from bow_match_cases import D, R, _filler
from fuse_cases import KfBuilder, pt

CHUNK = FC.CHUNK
LIMIT = 0.5
NONE = (-1, -1, -1, -1)
U, V = 100.5, 100.25        # the standard projection: cell (6, 6), its window of radius 2.5 stays inside that cell


def _case(name, frames, points, srch_kf, items, check, blocked=None, limits=None, th=1.0, th_on=False, eps=O.EPS_F64,
          marked=()):
    return dict(name=name, frames=[f.build() if isinstance(f, KfBuilder) else f for f in frames], blocked=blocked,
                pt_f64=np.array([p[0] for p in points], np.float64).reshape(-1, O.PT_F64),
                pt_desc=np.array([p[1] for p in points], np.uint8).reshape(-1, 32),
                limits=[LIMIT] * len(srch_kf) if limits is None else list(limits), srch_kf=list(srch_kf),
                items=[list(it) for it in items], th=th, th_on=th_on, eps=eps, check=check, marked=list(marked))


def arrays(case):
    return LO.join(case["frames"], case["blocked"], case["pt_f64"], case["pt_desc"], case["limits"], case["srch_kf"],
                   case["items"], case["th"], case["th_on"], case["eps"])


def oracle(case, **kw):
    return dict(zip(LO.OUTPUTS, LO.search(arrays(case), **kw)))


def geom(case, i, **kw):
    """The oracle's phase 1 of item i: (status, level, window or None)."""
    a = arrays(case)
    return LO._window(a, LO.search_of(a, i), i, **kw)[2]


def _expect(out, want, view=None, levels=None):
    """want: {item: (best_idx, best_dist, second_idx, second_dist)}, every other item has no candidate; view: the
    in_view flags (default: every item in view); levels: {item: level}."""
    n = len(out["status"])
    assert all(out[k].shape == (n,) for k in LO.OUTPUTS)
    for i in range(n):
        got = tuple(int(out[k][i]) for k in ("best_idx", "best_dist", "second_idx", "second_dist"))
        assert got == want.get(i, NONE), (i, got)
        assert int(out["in_view"][i]) == (1 if view is None else view[i]), (i, "in_view")
        assert (int(out["level"][i]) >= 0) == bool(out["in_view"][i])
    for i, lv in (levels or {}).items():
        assert int(out["level"][i]) == lv, (i, out["level"][i])


def _simple(name, kf, points, want, marked=(), view=None, levels=None, extra=None, **kw):
    """One search of every point into one frame."""
    c = _case(name, [kf], points, [0], [list(range(len(points)))], None, marked=marked, **kw)

    def check(out, c=c):
        _expect(out, want, view, levels)
        assert np.flatnonzero(out["status"]).tolist() == list(marked)
        if extra is not None:
            extra(c, out)
    c["check"] = check
    return c


def axis(c, level=0, desc=None, min_f=0.5, max_f=2.0):
    """(0.75, 0, 1) with the normal (0, 0, c): 1.25 away, at (48, 0), the viewing cosine exactly c / 1.25."""
    return [0.75, 0.0, 1.0, 0.0, 0.0, c, min_f * 1.25, max_f * 1.25, 1.25 * 1.25 ** (level - 0.5)], (
        D() if desc is None else desc)


def _one_feature(ur=-1.0):
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9), ur=ur)
    return kf


# ---- the launch shape -------------------------------------------------------------------------------------------------

def ragged_case(sizes, name):
    """Searches of the given item counts over a table of 80 points and a lattice frame of 20 features (row j looks at
    feature j % 20 from 3 + j // 20 bits away, a quarter of a pixel off, so that no window bound of radius 2.5 falls
    on a cell border); search s starts at row 7 s and walks the table with stride 3.  Nothing else is in a row's
    window, so there is no second."""
    kf = FC._lattice_kf(20)
    pts = [pt(50.25 + 40.0 * (j % 20 % 12), 60.25 + 40.0 * (j % 20 // 12), desc=D(*R(200, 200 + j // 20)))
           for j in range(80)]
    items = [[(7 * s + 3 * c) % 80 for c in range(n)] for s, n in enumerate(sizes)]
    want, i = {}, 0
    for it in items:
        for r in it:
            want[i] = (r % 20, 3 + r // 20, -1, -1)
            i += 1

    def check(out):
        assert len(out["status"]) == sum(sizes)
        _expect(out, want)
        assert not out["status"].any()
    return _case(name, [kf], pts, [0] * len(sizes), items, check)


def frames_case():
    """Three frames in one launch: the standard one, one without features and one that no search targets; two searches
    with different limits look at the same axis point of cosine 0.6."""
    a = KfBuilder()
    a.add(49.0, 1.0, D(1))
    p = axis(0.75)
    c = _case("two_limits_an_empty_frame_and_an_idle_one", [a, KfBuilder(), _one_feature()], [p, pt(U, V)], [0, 0, 1],
              [[0], [0], [0, 1]], None, limits=[0.5, 0.625, 0.5])

    def check(out, c=c):
        _expect(out, {0: (0, 1, -1, -1)}, view=[1, 0, 1, 1], levels={0: 0, 1: -1, 2: 0, 3: 0})
        assert geom(c, 0)[2][11] == 0.6 and 2 not in c["srch_kf"] and len(c["frames"][1]["xy"]) == 0
        assert not out["status"].any()
    c["check"] = check
    return c


# ---- the frustum gates --------------------------------------------------------------------------------------------------

def depth_case():
    """z = 0 is marked whatever x and y are; z = -2^-30 is behind the camera, unmarked and not in view, where
    k_fkf_search would go on; z = +2^-30 on the optical axis projects to (0, 0), where every bound is zero, and is in
    view."""
    tiny = 2.0 ** -30
    row = lambda x, y, z: ([x, y, z, 0.0, 0.0, 1.0, 0.0, 4.0, 1.0], D())  # noqa: E731
    kf = KfBuilder()
    kf.add(1.0, 1.0, D(9))
    near = ([0.0, 0.0, tiny, 0.0, 0.0, 1.0, 0.5 * tiny, 2.0 * tiny, tiny * 1.25 ** -0.5], D())

    def extra(c, out):
        assert geom(c, 2) == (0, -1, None) and geom(c, 4) == (0, -1, None)
        assert geom(c, 4, depth_gate=False)[1] == 0   # without the gate the mirrored point is in view
    p = pt(U, V)[0]
    mirrored = ([-x for x in p[:6]] + p[6:], D())
    return _simple("depth_zero_marked_behind_not_in_view_just_in_front_found", kf,
                   [row(0.0, 0.0, 0.0), row(1.0, 1.0, 0.0), row(0.0, 0.0, -tiny), near, mirrored],
                   {3: (0, 1, -1, -1)}, marked=[0, 1], view=[0, 0, 0, 1, 0], extra=extra)


def bound_cases():
    """Each image bound on the bound (inside, since both ends are inclusive, and marked, since u and v are rounded),
    half a pixel inside (found, unmarked) and half a pixel outside (not in view, unmarked)."""
    out = []
    for name, bounds, on, inside, outside, feat, cell in (
            ("u_on_max_x", (0.0, 640.0, 0.0, 480.0), (640.0, V), (639.5, V), (640.5, V), (639.0, 100.0), (39, 6)),
            ("u_on_min_x", (16.0, 640.0, 0.0, 480.0), (16.0, V), (16.5, V), (15.5, V), (17.0, 100.0), (0, 6)),
            ("v_on_max_y", (0.0, 640.0, 0.0, 480.0), (U, 480.0), (U, 479.5), (U, 480.5), (100.0, 479.0), (6, 29)),
            ("v_on_min_y", (0.0, 640.0, 16.0, 480.0), (U, 16.0), (U, 16.5), (U, 15.5), (100.0, 17.0), (6, 0))):
        kf = KfBuilder(bounds=bounds)
        kf.add(*feat, D(9), cell=cell)

        def extra(c, out_, on=on):
            assert geom(c, 0)[2][:2] == on and geom(c, 2) == (0, -1, None)
        out.append(_simple(name + "_is_inside_and_marked", kf, [pt(*on), pt(*inside), pt(*outside)],
                           {0: (0, 1, -1, -1), 1: (0, 1, -1, -1)}, marked=[0], view=[1, 1, 0], extra=extra))
    return out


def distance_case():
    """|p - Ow| exactly on the minimum and on the maximum invariance distance: both pass and both are marked.  A
    thousandth inside: unmarked and found.  A thousandth outside: not in view, unmarked."""
    pts = [pt(U, V, min_f=1.0), pt(U, V, max_f=1.0), pt(U, V, min_f=0.999), pt(U, V, max_f=1.001),
           pt(U, V, min_f=1.001), pt(U, V, max_f=0.999)]
    return _simple("distance_on_min_and_max_marked_outside_not_in_view", _one_feature(), pts,
                   {i: (0, 1, -1, -1) for i in range(4)}, marked=[0, 1], view=[1, 1, 1, 1, 0, 0])


def _on_0998():
    """A normal component c whose c / 1.25 is the double 0.998, or the nearest below it."""
    c = 0.998 * 1.25
    while c / 1.25 > 0.998:
        c = math.nextafter(c, 0.0)
    return c


def cosine_cases():
    """The viewing cosine on the limit (in view, marked), 2^-20 above (in view) and below (not in view); and around
    0.998, told by a feature 3 px away: above, the radius is 2.5 and it is outside; on (marked) and below, the radius is
    4 and it is found."""
    step = 2.0 ** -20
    kf = KfBuilder()
    kf.add(51.0, 1.0, D(9))
    lim = _simple("cosine_on_the_limit_marked_below_not_in_view", kf,
                  [axis(0.625), axis(0.625 + step), axis(0.625 - step)], {0: (0, 1, -1, -1), 1: (0, 1, -1, -1)},
                  marked=[0], view=[1, 1, 0],
                  extra=lambda c, out: _assert(geom(c, 0)[2][11] == 0.5 and geom(c, 0)[2][6] == 4.0))
    c0 = _on_0998()

    def extra(c, out):
        assert [geom(c, i)[2][6] for i in range(3)] == [4.0, 2.5, 4.0]
        assert abs(geom(c, 0)[2][11] - 0.998) < 2.0 ** -50 and not geom(c, 0)[2][11] > 0.998
    rad = _simple("cosine_on_0998_marked_radius_4_above_radius_2_5", kf, [axis(c0), axis(c0 + step), axis(c0 - step)],
                  {0: (0, 1, -1, -1), 2: (0, 1, -1, -1)}, marked=[0], extra=extra)
    return [lim, rad]


def _assert(cond):
    assert cond


def level_cases():
    """The level quotient on an integer is marked; a thousandth below it is level 1, above it level 2.  Quotients -2.5
    and 7.5 clamp to levels 0 and 3."""
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9), octave=1)
    on = _simple("level_quotient_on_an_integer_marked", kf, [pt(U, V, q=1.0), pt(U, V, q=0.999), pt(U, V, q=1.001)],
                 {0: (0, 1, -1, -1), 1: (0, 1, -1, -1), 2: (0, 1, -1, -1)}, marked=[0], levels={1: 1, 2: 2})
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9), octave=0)
    kf.add(101.0, 100.0, D(9, 10), octave=3)
    clamp = _simple("level_clamped_low_and_high", kf, [pt(U, V, q=-2.5), pt(U, V, q=7.5)],
                    {0: (0, 1, -1, -1), 1: (1, 2, -1, -1)}, levels={0: 0, 1: 3})
    return [on, clamp]


# ---- the radius ---------------------------------------------------------------------------------------------------------

def th_cases():
    """A feature exactly 2.5 px away.  th = 1 with the flag off: r = 2.5, outside, and marked.  th = 1.0000001 with the
    flag on: r = 2.50000025, inside, unmarked.  th = 1.0000001 with the flag off: th is not read, as with th = 1."""
    out = []
    for name, th, on, want, marked in (("th_1_flag_off", 1.0, False, {}, [0]),
                                       ("th_1_0000001_flag_on", 1.0000001, True, {0: (0, 1, -1, -1)}, []),
                                       ("th_1_0000001_flag_off_is_not_read", 1.0000001, False, {}, [0]),
                                       ("th_5_flag_on", 5.0, True, {0: (0, 1, -1, -1)}, [])):
        kf = KfBuilder()
        kf.add(U + 2.5, V, D(9), cell=(6, 6))
        r = 2.5 * th if on else 2.5
        out.append(_simple(name, kf, [pt(U, V)], want, marked=marked, th=th, th_on=on,
                           extra=lambda c, o, r=r: _assert(geom(c, 0)[2][6] == r)))
    return out


def stereo_case():
    """ur = 68.5 and r = 2.5.  Features in the window with right coordinates ur + r (kept: the gate is er > r; marked),
    ur + r - 1/4 (kept), ur + r + 1/4 (left out), and 0 and -1 (no gate, however far ur is).  Each point sees one
    feature, in a cell of its own."""
    urs = [71.0, 70.75, 71.25, 0.0, -1.0]
    kf = KfBuilder()
    pts, want = [], {}
    for j, kr in enumerate(urs):
        kf.add(100.0, 100.0 + 32.0 * j, D(9), ur=kr)
        pts.append(pt(U, V + 32.0 * j))
        if kr != 71.25:
            want[j] = (j, 1, -1, -1)

    def extra(c, out):
        assert geom(c, 0)[2][2] == 68.5
        free = oracle(c, stereo_gate=False)
        assert int(free["best_idx"][2]) == 2 and not free["status"].any()
    return _simple("stereo_gate_on_below_above_and_ungated", kf, pts, want, marked=[0], extra=extra)


# ---- best and second ----------------------------------------------------------------------------------------------------

def _cell_kf(descs, octaves=None, urs=None):
    """Features in one cell, (6, 6), in the given stored order, all within 2.5 px of (U, V)."""
    kf = KfBuilder()
    for j, d in enumerate(descs):
        kf.add(U - 2.0 + 0.125 * (j % 32), V - 0.75 + 0.25 * (j % 7), d, octave=0 if octaves is None else octaves[j],
               ur=-1.0 if urs is None else urs[j], cell=(6, 6))
    return kf


def window_cases():
    """15, 16 and 17 candidates in one cell, so one run of the 16 lanes, exactly one, and one plus one entry: the best
    is the last visited, the second the first."""
    out = []
    for L in (15, 16, 17):
        descs = [D(1, 2, 3)] + [_filler(j) for j in range(1, L - 1)] + [D(1, 2)]
        out.append(_simple(f"window_{L}", _cell_kf(descs), [pt(U, V)], {0: (L - 1, 2, 0, 3)},
                           extra=lambda c, o, L=L: _assert(len(LO.candidates(arrays(c), 0, 0)[3]) == L)))
    return out


def lane_cases():
    """Of 20 candidates in one cell entry j is taken by lane j % 16.  Best at 16 and second at 0: one lane holds both.
    Best at 5 and second at 9: two lanes.  Second in the lane of the best, third elsewhere and closer than the best's
    lane mate: the reduction must not take a lane's first for the second."""
    def kf_of(where):
        return _cell_kf([where.get(j, _filler(j)) for j in range(20)])
    one = _simple("best_and_second_in_one_lane", kf_of({16: D(1), 0: D(1, 2)}), [pt(U, V)], {0: (16, 1, 0, 2)})
    two = _simple("best_and_second_in_two_lanes", kf_of({5: D(1), 9: D(1, 2)}), [pt(U, V)], {0: (5, 1, 9, 2)})
    mix = _simple("second_is_the_best_lanes_other_entry", kf_of({3: D(1), 19: D(1, 2), 7: D(1, 2, 3)}), [pt(U, V)],
                  {0: (3, 1, 19, 2)})
    return [one, two, mix]


def tie_cases():
    """Equal distances: the earliest visited is best and the next visited second, in one lane's entries (2 and 18), in
    two lanes, and across two cells (column 6 before column 7); three equal ones leave the third out."""
    eq = D(1, 2)
    same = _simple("tie_in_one_lane", _cell_kf([eq if j in (2, 18) else _filler(j) for j in range(20)]), [pt(U, V)],
                   {0: (2, 2, 18, 2)})
    lanes = _simple("tie_of_three_in_three_lanes", _cell_kf([D(3, 4) if j in (4, 6, 11) else _filler(j)
                                                            for j in range(20)]), [pt(U, V)], {0: (4, 2, 6, 2)})
    kf = KfBuilder()
    kf.add(112.5, 100.0, D(1, 2))   # index 0 in column 7: visited after column 6
    kf.add(111.5, 100.0, D(3, 4))   # index 1 in column 6
    cells = _simple("tie_in_two_cells", kf, [pt(112.0, V)], {0: (1, 2, 0, 2)})
    return [same, lanes, cells]


def single_case():
    return _simple("single_candidate_has_no_second", _one_feature(), [pt(U, V)], {0: (0, 1, -1, -1)})


def octave_cases():
    """Level 2: octaves 0 and 3 hold closer descriptors and are left out, and the second best sits on the other
    admitted octave.  Level 0: the lowest admitted octave is -1, and octave 1 is left out."""
    two = _simple("octaves_two_below_and_one_above_left_out_second_on_the_other_octave",
                  _cell_kf([D(1), D(1, 2), D(1, 2, 3), D(1, 2, 3, 4)], octaves=[0, 3, 2, 1]), [pt(U, V, level=2)],
                  {0: (2, 3, 3, 4)}, levels={0: 2},
                  extra=lambda c, o: _assert(int(oracle(c, three_octaves=True)["best_idx"][0]) == 1))
    zero = _simple("level_0_takes_octave_0_only", _cell_kf([D(1), D(1, 2)], octaves=[1, 0]), [pt(U, V)],
                   {0: (1, 2, -1, -1)}, levels={0: 0})
    return [two, zero]


def blocked_cases():
    """Three candidates 1, 2 and 3 bits away.  The best blocked: second and third move up.  The second blocked: the
    third is second.  The third blocked: nothing changes.  A blocked entry marks nothing: the blocked feature of the
    last case lies exactly one radius away."""
    descs = [D(1), D(1, 2), D(1, 2, 3)]
    out = []
    for name, blk, want in (("blocked_best", [1, 0, 0], (1, 2, 2, 3)), ("blocked_second", [0, 1, 0], (0, 1, 2, 3)),
                            ("blocked_third_changes_nothing", [0, 0, 1], (0, 1, 1, 2))):
        out.append(_simple(name, _cell_kf(descs), [pt(U, V)], {0: want}, blocked=[blk],
                           extra=lambda c, o: _assert(tuple(int(oracle(c, blocked=False)[k][0]) for k in (
                               "best_idx", "second_idx")) == (0, 1))))
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1))
    kf.add(U + 2.5, V, D(1, 2), cell=(6, 6))
    out.append(_simple("blocked_entry_marks_nothing", kf, [pt(U, V)], {0: (0, 1, -1, -1)}, blocked=[[0, 1]],
                       extra=lambda c, o: _assert(oracle(c, blocked=False)["status"].tolist() == [O.MARGINAL])))
    return out


def radius_case():
    """r = 2.5: the closer descriptor is 2.75 px away, the other 2.25 px."""
    kf = KfBuilder()
    kf.add(U + 2.75, V, D(1), cell=(6, 6))
    kf.add(U + 2.25, V, D(1, 2, 3), cell=(6, 6))
    return _simple("feature_just_inside_and_just_outside_the_radius", kf, [pt(U, V)], {0: (1, 3, -1, -1)})


def window_edge_cases():
    """Both ends truncate: (100.5 + 2.5) / 16 = 6.4 is column 6, and a feature stored in column 7 is not visited.  A
    grid of 10 x 10 cells in the same image: a point in view beyond it has a level and no window."""
    kf = KfBuilder()
    kf.add(101.0, 100.0, D(1), cell=(7, 6))
    kf.add(100.0, 100.0, D(1, 2, 3), cell=(6, 6))
    trunc = _simple("upper_end_truncates", kf, [pt(U, V)], {0: (1, 3, -1, -1)},
                    extra=lambda c, o: _assert(geom(c, 0)[2][7:9] == (6, 6)))
    kf = KfBuilder(cols=10, rows=10)
    kf.add(100.0, 100.0, D(9))
    beyond = _simple("in_view_without_a_window", kf, [pt(300.5, V), pt(U, 300.25)], {}, levels={0: 0, 1: 0},
                     extra=lambda c, o: _assert(geom(c, 0) == (0, 0, None)))
    return [trunc, beyond]


def eps_cases():
    """A feature 2^-30 of a pixel inside the radius: float32's unit of rounding marks it, float64's does not."""
    kf = KfBuilder()
    kf.add(U + 2.5 - 2.0 ** -30, V, D(1), cell=(6, 6))
    return [_simple("eps_of_float32_marks_what_float64_does_not", kf, [pt(U, V)], {0: (0, 1, -1, -1)}, marked=[0],
                    eps=O.EPS_F32),
            _simple("eps_of_float64_leaves_it_unmarked", kf, [pt(U, V)], {0: (0, 1, -1, -1)}, eps=O.EPS_F64)]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = ([ragged_case((1, 0, 255, 256, 0, 257, 0), "ragged_0_1_255_256_257"), ragged_case((0, 0), "zero_items"),
                 ragged_case((), "zero_searches"), frames_case(), depth_case()] + bound_cases() + [distance_case()]
                + cosine_cases() + level_cases() + th_cases() + [stereo_case()] + window_cases() + lane_cases()
                + tie_cases() + [single_case()] + octave_cases() + blocked_cases() + [radius_case()]
                + window_edge_cases() + eps_cases())
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


# ---- Tracking.search_local_points on a matcher_world world (shared by the golden's generator and the tests) ---------

class MapPoint(MW.MapPoint):
    """matcher_world's MapPoint with what Tracking.search_local_points and Frame.is_in_frustum touch besides
    (MapPoint.py): mnLastFrameSeen, mbTrackInView, mnVisible and increase_visible, and observations() as a stored
    count."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.mnLastFrameSeen = -1
        self.mbTrackInView = False
        self.mnVisible = 1
        self.nObs = 0

    def observations(self):
        return self.nObs

    def increase_visible(self, n=1):
        self.mnVisible += n


class Frame(KC.Frame):
    """fkf_cases' Frame with the pose parts Frame.set_pose derives (Frame.py:127-135) and an id."""

    def __init__(self, world, a, Tcw, mn_id=7):
        super().__init__(world, a, Tcw)
        self.mnId = mn_id
        self.set_pose(Tcw)

    def set_pose(self, Tcw):
        self.mTcw = Tcw.copy()
        self.mRcw = self.mTcw[:3, :3]
        self.mRwc = self.mRcw.T
        self.mtcw = self.mTcw[:3, 3].reshape(3, 1)
        self.mOw = -np.dot(self.mRwc, self.mtcw)


ATTRS = ("mTrackProjX", "mTrackProjY", "mTrackProjXR", "mTrackViewCos")
# pose and position dtype, th, nnratio
CONFIGS = ((np.float64, 1, 0.8), (np.float32, 1, 0.8), (np.float64, 5, 1), (np.float32, 5, 1), (np.float64, 5, 0.8),
           (np.float32, 1, 1))
N_FRAMES = 2


def make_extras(z, seed, n_stale=2, n_seen=5, n_pre=60, n_dup=12, obs_share=0.1):
    """What the golden adds to a fuse_cases.clone_world (changed in place), per frame k < N_FRAMES, whose features
    are keyframe 5 + k's: ls_T{k}, its pose (that keyframe's, moved a little); ls_local{k}, the local map (map point
    ids, shuffled); ls_seen{k}, those already seen in the frame; ls_stale{k}, seen ones that still carry a stale
    projection (ls_stale_xy{k}: px, py, pxr, level, cosine); ls_obs, observations() per map point (0, 1 or 2);
    ls_pre{k}, the frame's slots before the call.  In each frame n_dup features that re-observe a map point get a
    near copy (a pixel away, the same octave, a descriptor two bits away, no right coordinate) in place of a feature
    that re-observes nothing, so best and second lie close together and the ratio test has something to reject.  A
    tenth of the points have observations: each assignment by one of them takes a feature away from the items after
    it, and with more of them the share of items redone alone passes the 5 % the tests allow."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_mp = len(z["mp_desc"])
    z["ls_obs"] = np.where(rng.random(n_mp) < obs_share, rng.integers(1, 3, n_mp), 0).astype(np.int32)
    for k in range(N_FRAMES):
        kf = 5 + k
        T = z[f"kf{kf}_T"].copy()
        T[:3, 3] += rng.normal(0, 0.02, 3).astype(np.float32)
        z[f"ls_T{k}"] = T
        held = np.unique(np.concatenate([z[f"kfmp{j}"][z[f"kfmp{j}"] >= 0] for j in range(5 + N_FRAMES)]))
        local = rng.permutation(held).astype(np.int32)
        z[f"ls_local{k}"] = local
        seen = rng.choice(local, n_seen, replace=False).astype(np.int32)
        z[f"ls_seen{k}"] = seen
        stale = seen[:n_stale]
        z[f"ls_stale{k}"] = stale
        n = len(z[f"kf{kf}_x"])
        f = rng.choice(n, n_stale, replace=False)
        xy = np.zeros((n_stale, 5))
        xy[:, 0] = z[f"kf{kf}_x"][f] + rng.normal(0, 0.7, n_stale)
        xy[:, 1] = z[f"kf{kf}_y"][f] + rng.normal(0, 0.7, n_stale)
        xy[:, 2] = xy[:, 0] - rng.uniform(5, 40, n_stale)
        xy[:, 3] = z[f"kf{kf}_octave"][f]
        xy[:, 4] = rng.uniform(0.9, 1.0, n_stale)
        z[f"ls_stale_xy{k}"] = xy
        slots = z[f"kfmp{kf}"]
        src = rng.choice(np.flatnonzero(slots >= 0), n_dup, replace=False)
        dst = rng.choice(np.flatnonzero(slots < 0), n_dup, replace=False)
        for a_, b_ in zip(src.tolist(), dst.tolist()):
            z[f"kf{kf}_x"][b_] = z[f"kf{kf}_x"][a_] + np.float32(rng.choice([-1.0, 1.0]))
            z[f"kf{kf}_y"][b_] = z[f"kf{kf}_y"][a_] + np.float32(rng.choice([-0.5, 0.5]))
            z[f"kf{kf}_octave"][b_] = z[f"kf{kf}_octave"][a_]
            z[f"kf{kf}_desc"][b_] = MW.noisy_desc(rng, z[f"kf{kf}_desc"][a_], 2)
            z[f"kf{kf}_uR"][b_] = -1.0
        pre = np.full(n, -1, np.int32)
        for i in rng.choice(n, n_pre, replace=False).tolist():
            pre[i] = slots[i] if slots[i] >= 0 else int(rng.integers(n_mp))
        z[f"ls_pre{k}"] = pre
    return z


def build(g, dtype):
    """A fresh world of the golden's arrays with MapPoint / Frame above, poses and positions of the given dtype:
    [(frame, local map list)] per frame, and the world."""
    w = MW.World()
    for i in range(len(g["mp_desc"])):
        p = MapPoint(w, i, g["mp_pos"][i], g["mp_desc"][i], g["mp_normal"][i], g["mp_min"][i], g["mp_max"][i],
                     bool(g["mp_bad"][i]))
        p._pos, p._normal = p._pos.astype(dtype), p._normal.astype(dtype)
        p.nObs = int(g["ls_obs"][i])
        w.mps.append(p)
    jobs = []
    for k in range(N_FRAMES):
        F = Frame(w, MW.sub(g, f"kf{5 + k}_"), g[f"ls_T{k}"].astype(dtype), mn_id=40 + k)
        F.mvpMapPoints = [w.mps[int(m)] if m >= 0 else None for m in g[f"ls_pre{k}"]]
        jobs.append((F, [w.mps[int(m)] for m in g[f"ls_local{k}"]]))
    return jobs, w


def prepare(g, jobs, w, k, dtype):
    """What Tracking leaves before frame k's search_local_points: the seen points marked, the stale ones with the
    projection an earlier frame left (arrays of the shapes is_in_frustum leaves)."""
    F = jobs[k][0]
    for m in g[f"ls_seen{k}"]:
        w.mps[int(m)].mnLastFrameSeen = F.mnId
    for m, (px, py, pxr, lv, vc) in zip(g[f"ls_stale{k}"], g[f"ls_stale_xy{k}"]):
        p = w.mps[int(m)]
        p.mbTrackInView = True
        p.mTrackProjX, p.mTrackProjY = np.array([px], dtype), np.array([py], dtype)
        p.mTrackProjXR, p.mnTrackScaleLevel = np.array([pxr], dtype), int(lv)
        p.mTrackViewCos = np.array([[vc]], dtype)


def snapshot(w, jobs):
    """Everything a call leaves behind: the frames' slots; per map point mbTrackInView, mnVisible, the level, and the
    four projections' values, dtypes and shapes (NaN / -1 where the point has none)."""
    n = len(w.mps)
    view = np.array([bool(p.mbTrackInView) for p in w.mps])
    vis = np.array([p.mnVisible for p in w.mps], np.int32)
    lvl = np.array([getattr(p, "mnTrackScaleLevel", -1) for p in w.mps], np.int32)
    val = np.full((n, 4), np.nan)
    kind = np.full((n, 4), -1, np.int32)   # itemsize * 10 + ndim
    for i, p in enumerate(w.mps):
        for c, name in enumerate(ATTRS):
            a = getattr(p, name, None)
            if a is not None:
                assert type(a) is np.ndarray and a.size == 1, (name, type(a))
                val[i, c], kind[i, c] = float(a.reshape(-1)[0]), a.dtype.itemsize * 10 + a.ndim
    return dict(slots=np.stack([MW.encode_mps(w, F.mvpMapPoints) for F, _ in jobs]), view=view, vis=vis, lvl=lvl,
                val=val, kind=kind)


def drive(g, run, cfg):
    """The N_FRAMES calls of a configuration on a fresh world through run(jobs, th, limit, nnratio, prepare) ->
    [(nToMatch, n)], where prepare(k) must be called right before frame k's search: (the results as an (N_FRAMES, 2)
    array with -1 for None, the snapshot)."""
    dtype, th, nn = CONFIGS[cfg]
    jobs, w = build(g, dtype)
    res = run(jobs, th, LIMIT, nn, lambda k: prepare(g, jobs, w, k, dtype))
    return np.array([[a, -1 if b is None else b] for a, b in res], np.int32), snapshot(w, jobs)


def prepare_all(jobs, prep):
    for k in range(len(jobs)):
        prep(k)


def by_loop(frustum, f_p):
    """The loop of the issue with the given is_in_frustum(F, pMP, limit) and f_p(F, vp, th, nnratio)."""
    def run(jobs, th, limit, nn, prep):
        prepare_all(jobs, prep)
        out = []
        for F, vp in jobs:
            n_to_match = 0
            for pMP in vp:
                if pMP.mnLastFrameSeen == F.mnId:
                    continue
                if pMP.is_bad():
                    continue
                if frustum(F, pMP, limit):
                    pMP.increase_visible()
                    n_to_match += 1
            out.append((n_to_match, f_p(F, vp, th, nn) if n_to_match > 0 else None))
        return out
    return run


def by_oracle(stats=None, results=None):
    def run(jobs, th, limit, nn, prep):
        prepare_all(jobs, prep)
        return LO.replay(jobs, th, limit, nn, results=results, stats=stats)
    return run


def by_matcher(matcher_cls, many=False):
    def run(jobs, th, limit, nn, prep):
        prepare_all(jobs, prep)
        m = matcher_cls(nn, True)
        if many:
            return m.search_local_points_many([j[0] for j in jobs], [j[1] for j in jobs], th, limit)
        return [m.search_local_points(F, vp, th, limit) for F, vp in jobs]
    return run


def golden_results(g, cfg):
    return g[f"ls_res{cfg}"], {k: g[f"ls_{k}{cfg}"] for k in ("slots", "view", "vis", "lvl", "val", "kind")}


def same(got, want):
    """Results and snapshots equal, NaN for NaN."""
    return np.array_equal(got[0], want[0]) and all(
        np.array_equal(got[1][k], want[1][k], equal_nan=(k == "val")) for k in want[1])


def diff(got, want):
    return [k for k in want[1] if not np.array_equal(got[1][k], want[1][k], equal_nan=(k == "val"))] + (
        [] if np.array_equal(got[0], want[0]) else ["res"])
