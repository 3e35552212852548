"""Cases for k_ff_search on the geometry of tests/fuse_cases.py (identity pose, fx = fy = 64, cx = cy = 0, bf = 32, the
image [0, 640] x [0, 480], 16 px cells, four levels with the scale factors 1, 1.25, 1.5, 2): a point made by `pt(u, v)`
lies at depth 1 and lands on exactly (u, v) with ur = u - 32; slots 3-8 of its row hold NaN, which the search never
reads.  th is 3 and the mode 0 unless a case says otherwise, so a level-0 item has the radius 3.

A search is a target frame, a th, an octave mode and a list of (row of one shared point table, level); a frame has one
blocked byte and one right coordinate per feature.  Each case carries its claim as a `check` over the array oracle's
results (a dict by output name), which tests/test_ff_cases_cpu.py runs, so the GPU test that compares the kernel with
the oracle cannot pass on inputs that miss the situation.

A case: name, frames (fuse_oracle keyframe dicts), blocked (per frame, or None), pt_f64 / pt_desc (the point table),
ths / modes / srch_kf / items / levels (per search its th, its mode, its target, its rows of the table and their
levels), eps, check(out) and marked (the items built to come back ORBFE_FUSE_MARGINAL; no other item may).

Also the stand-ins with the surface ORBMatcher.search_by_projection_f_f reads, and the loader and drivers of the golden
tests/golden/ff_many.npz, shared by its generator and the tests.
"""
from __future__ import annotations

import math

import numpy as np

import ff_oracle as FO
import fuse_cases as FC
import matcher_frames as MF
from bow_match_cases import D, R
from fuse_cases import KfBuilder

CHUNK = FC.CHUNK
TH = 3.0
NAN = float("nan")
U, V = 100.5, 100.25        # the standard projection: cell (6, 6), its window of radius 3 stays inside that cell


def pt(u, v, z=1.0, desc=None):
    """A point that projects to exactly (u, v) in the standard frame from depth z (a power of two, or negative)."""
    return [u * z / FC.FX, v * z / FC.FY, z] + [NAN] * 6, (D() if desc is None else desc)


def _case(name, frames, points, srch_kf, items, check, levels=None, ths=None, modes=None, blocked=None,
          eps=FO.EPS_F64, marked=()):
    items = [list(it) for it in items]
    return dict(name=name, frames=[f.build() if isinstance(f, KfBuilder) else f for f in frames], blocked=blocked,
                pt_f64=np.array([p[0] for p in points], np.float64).reshape(-1, FO.PT_F64),
                pt_desc=np.array([p[1] for p in points], np.uint8).reshape(-1, 32),
                ths=[TH] * len(srch_kf) if ths is None else list(ths),
                modes=[0] * len(srch_kf) if modes is None else list(modes), srch_kf=list(srch_kf), items=items,
                levels=[[0] * len(it) for it in items] if levels is None else [list(lv) for lv in levels], eps=eps,
                check=check, marked=list(marked))


def arrays(case):
    return FO.join(case["frames"], case["blocked"], case["pt_f64"], case["pt_desc"], case["ths"], case["modes"],
                   case["srch_kf"], case["items"], case["levels"], case["eps"])


def oracle(case, **kw):
    return dict(zip(FO.OUTPUTS, FO.search(arrays(case), **kw)))


def geom(case, i, **kw):
    """The oracle's phase 1 of item i: (status, window or None)."""
    a = arrays(case)
    return FO._window(a, FO.search_of(a, i), i, **kw)[2]


def cands(case, i, **kw):
    """The features item i may take, in visiting order."""
    a = arrays(case)
    return [c[2] for c in FO.candidates(a, FO.search_of(a, i), i, **kw)[1]]


def _expect(out, want):
    """want: {item: (best_idx, best_dist)}, every other item has no candidate."""
    n = len(out["status"])
    assert all(out[k].shape == (n,) for k in FO.OUTPUTS)
    for i in range(n):
        got = (int(out["best_idx"][i]), int(out["best_dist"][i]))
        assert got == want.get(i, (-1, -1)), (i, got)


def _with(c, want, extra=None):
    def check(out, c=c):
        _expect(out, want)
        assert np.flatnonzero(out["status"]).tolist() == c["marked"]
        if extra is not None:
            extra(c, out)
    c["check"] = check
    return c


def _simple(name, kf, points, want, marked=(), levels=None, th=TH, mode=0, extra=None, **kw):
    """One search of every point into one frame."""
    c = _case(name, [kf], points, [0], [list(range(len(points)))], None, marked=marked, ths=[th], modes=[mode],
              levels=None if levels is None else [levels], **kw)
    return _with(c, want, extra)


def _assert(cond):
    assert cond


def _one_feature(ur=-1.0, octave=0):
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9), ur=ur, octave=octave)
    return kf


# ---- the launch shape -------------------------------------------------------------------------------------------------

def ragged_case(sizes, name):
    """Searches of the given sizes into one frame of 20 features; item n looks at feature n % 20 and differs from it in
    3 + n % 4 bits."""
    kf = FC._lattice_kf(20)
    pts, items, want, n = [], [], {}, 0
    for size in sizes:
        it = []
        for _ in range(size):
            j = n % 20
            it.append(len(pts))
            pts.append(pt(50.5 + 40.0 * (j % 12), 60.25 + 40.0 * (j // 12), desc=D(*R(200, 200 + n % 4))))
            want[n] = (j, 3 + n % 4)
            n += 1
        items.append(it)
    c = _case(name, [kf], pts, [0] * len(sizes), items, None)
    return _with(c, want, lambda c, out: _assert(len(out["status"]) == sum(sizes)))


def two_searches_case():
    """Two searches into one frame with the same item: th 3 in mode 0 sees the near feature of octave 0 only (the far
    one lies 4 px off, beyond 3.75); th 6 in the forward mode sees the far feature of octave 2 only."""
    kf = KfBuilder()
    kf.add(101.0, 100.0, D(1), octave=0)
    kf.add(104.5, 100.0, D(1, 2), octave=2)
    c = _case("two_searches_one_frame_two_ths_two_modes", [kf], [pt(U, V)], [0, 0], [[0], [0]], None,
              levels=[[1], [1]], ths=[3.0, 6.0], modes=[0, 1])
    return _with(c, {0: (0, 1), 1: (1, 2)},
                 lambda c, out: _assert(cands(c, 0) == [0] and cands(c, 1) == [1] and cands(c, 1, mode=0) == [0, 1]))


def frames_case():
    """Three frames: one with features that no search targets, an empty one that is searched, and the standard one."""
    idle = KfBuilder()
    idle.add(100.0, 100.0, D(5))
    c = _case("an_empty_frame_and_an_untargeted_one", [idle, KfBuilder(), _one_feature()], [pt(U, V)], [1, 2],
              [[0], [0]], None)
    return _with(c, {1: (0, 1)}, lambda c, out: _assert(0 not in c["srch_kf"] and len(c["frames"][1]["xy"]) == 0))


# ---- depth ------------------------------------------------------------------------------------------------------------

def depth_cases():
    """pc.z < 0 is skipped without a mark although it projects onto the feature; within its bound of zero it is marked;
    pc.z == +0 and -0 are marked and get no candidate."""
    behind = _simple("behind_the_camera_is_skipped", _one_feature(), [pt(U, V), pt(U, V, z=-1.0)], {0: (0, 1)},
                     extra=lambda c, out: _assert(geom(c, 1) == (0, None)
                                                  and geom(c, 1, depth_gate=False)[1][:2] == (U, V)))
    # t = (0, 0, 1): pc.z = p.z + 1 and its bound is 4 eps (|p.z| + 1) = 2^-20 for float32's eps
    kf = KfBuilder(t=(0.0, 0.0, 1.0))
    kf.add(100.0, 100.0, D(9))
    pts = [([0.0, 0.0, -1.0 - 2.0 ** -40] + [NAN] * 6, D()), ([0.0, 0.0, -1.0] + [NAN] * 6, D()),
           ([0.0, 0.0, -1.0 + 2.0 ** -40] + [NAN] * 6, D()), ([0.0, 0.0, -1.5] + [NAN] * 6, D())]
    near = _simple("depth_within_its_bound_of_zero_is_marked", kf, pts, {}, marked=[0, 1, 2], eps=FO.EPS_F32)
    # every term of pc.z is a negative zero: the sum is -0.0, whose reciprocal is -inf
    kf = KfBuilder(t=(0.0, 0.0, -0.0))
    kf.add(100.0, 100.0, D(9))
    zero = _simple("depth_of_either_zero_is_marked", kf,
                   [([-1.0, -1.0, -0.0] + [NAN] * 6, D()), ([1.0, 1.0, 0.0] + [NAN] * 6, D())], {}, marked=[0, 1],
                   extra=lambda c, out: _assert(math.copysign(1.0, _zc(c, 0)) == -1.0 and _zc(c, 0) == 0.0
                                                and math.copysign(1.0, _zc(c, 1)) == 1.0))
    return [behind, near, zero]


def _zc(c, i):
    K, P = c["frames"][0]["f64"], c["pt_f64"][i]
    return float(((K[11] * P[0] + K[12] * P[1]) + K[13] * P[2]) + K[16])


# ---- projection and window ----------------------------------------------------------------------------------------------

def order_case():
    """fx = 63 here, no power of two: (fx * xc) * invz and fx * (xc * invz) differ in the last place at depth 3, and a
    feature exactly one radius from the second is inside for the first.  The item is marked either way; the candidate
    lists differ."""
    fx, z, iz = 63.0, 3.0, 1.0 / 3.0
    for n in range(1, 4000):
        xc = 3.0 + n / 64.0
        u1, u2 = (fx * xc) * iz, fx * (xc * iz)
        kx = u2 + TH
        if u1 != u2 and kx - u2 == TH and abs(kx - u1) < TH:
            kf = KfBuilder()
            kf.add(kx, 100.0, D(9), cell=(int(kx // 16), 6))
            frame = kf.build()
            frame["f64"][0] = fx
            p = ([xc, 100.25 * z / 64.0, z] + [NAN] * 6, D())
            return _simple("multiplication_order_decides", frame, [p], {0: (0, 1)}, marked=[0],
                           extra=lambda c, out: _assert(cands(c, 0) == [0] and cands(c, 0, fkf_order=False) == []
                                                        and geom(c, 0)[1][0] == u1))
    raise AssertionError("no such point")


def bound_cases():
    """Each image bound on the bound (inside, since both ends are inclusive, and marked, since u and v are rounded),
    half a pixel inside (found, unmarked) and half a pixel outside (no search, unmarked)."""
    out = []
    for name, bounds, on, inside, outside, feat, cell in (
            ("u_on_max_x", (0.0, 640.0, 0.0, 480.0), (640.0, V), (639.5, V), (640.5, V), (639.0, 100.0), (39, 6)),
            ("u_on_min_x", (16.0, 640.0, 0.0, 480.0), (16.0, V), (16.5, V), (15.5, V), (17.0, 100.0), (0, 6)),
            ("v_on_max_y", (0.0, 640.0, 0.0, 480.0), (U, 480.0), (U, 479.5), (U, 480.5), (100.0, 479.0), (6, 29)),
            ("v_on_min_y", (0.0, 640.0, 16.0, 480.0), (U, 16.0), (U, 16.5), (U, 15.5), (100.0, 17.0), (6, 0))):
        kf = KfBuilder(bounds=bounds)
        kf.add(*feat, D(9), cell=cell)
        out.append(_simple(name + "_is_inside_and_marked", kf, [pt(*on), pt(*inside), pt(*outside)],
                           {0: (0, 1), 1: (0, 1)}, marked=[0],
                           extra=lambda c, o, on=on: _assert(geom(c, 0)[1][:2] == on and geom(c, 2) == (0, None))))
    return out


def window_cases():
    """A lower end in (-1, 0) is cell 0 and marks nothing; both ends truncate, so a feature stored one column up is not
    visited; the clamp at the last column; the four early returns, in a grid of 10 x 10 cells in the same image and
    with th = -20, whose upper end is at most -1."""
    kf = KfBuilder()
    kf.add(0.5, 100.0, D(9))
    out = [_simple("lower_end_between_minus_one_and_zero_is_cell_zero", kf, [pt(2.0, V)], {0: (0, 1)},
                   extra=lambda c, o: _assert(geom(c, 0)[1][7:9] == (0, 0)))]
    kf = KfBuilder()
    kf.add(101.0, 100.0, D(1), cell=(7, 6))
    kf.add(100.0, 100.0, D(1, 2, 3), cell=(6, 6))
    out.append(_simple("upper_end_truncates", kf, [pt(U, V)], {0: (1, 3)},
                       extra=lambda c, o: _assert(geom(c, 0)[1][7:9] == (6, 6))))
    kf = KfBuilder()
    kf.add(637.0, 100.0, D(9))
    out.append(_simple("clamp_col_last", kf, [pt(638.5, V)], {0: (0, 1)},
                       extra=lambda c, o: _assert(geom(c, 0)[1][7:9] == (39, 39))))
    for name, (u, v), th in (("x0", (300.5, V), TH), ("x1", (2.0, V), -20.0), ("y0", (U, 300.25), TH),
                             ("y1", (U, 2.0), -20.0)):
        kf = KfBuilder(cols=10, rows=10)
        kf.add(100.0, 100.0, D(9))

        def extra(c, o, name=name, u=u, v=v, th=th):
            assert geom(c, 0) == (0, None)
            raw = dict(x0=int((u - th) / 16) >= 10, x1=int((u + th) / 16) < 0, y0=int((v - th) / 16) >= 10,
                       y1=int((v + th) / 16) < 0)
            assert [k for k, hit in raw.items() if hit] == [name]
        out.append(_simple(f"early_return_{name}", kf, [pt(u, v)], {}, th=th, extra=extra))
    return out


# ---- the octave modes ---------------------------------------------------------------------------------------------------

def octave_cases():
    """Four features of octaves 3, 2, 1, 0 in one cell in that order, all at the same place and the same distance, and
    two items of levels 2 and 1 (so the octaves level - 2 ... level + 2 all occur), in each mode: the first stored of
    the allowed octaves wins.  Then level 0 and level 3 in mode 0 and in the forward mode.  The point lands 2.5 px
    from the features, so that no window end of the radii 3, 3.75, 4.5 and 6 falls on a cell border."""
    def kf4():
        kf = KfBuilder()
        for o in (3, 2, 1, 0):
            kf.add(100.0, 100.0, D(1), octave=o)   # feature index 3 - octave
        return kf
    c = _case("octaves_around_the_level_in_three_modes", [kf4()], [pt(102.5, V)], [0, 0, 0], [[0, 0]] * 3, None,
              levels=[[2, 1]] * 3, modes=[0, 1, 2])
    allowed = {0: [3, 2, 1], 1: [2, 1, 0], 2: [3, 2], 3: [3, 2, 1], 4: [2, 1, 0], 5: [1, 0]}   # octaves, per item
    _with(c, {i: (3 - a[0], 1) for i, a in allowed.items()},
          lambda c, out: _assert(all(cands(c, i) == [3 - o for o in a] for i, a in allowed.items())))
    e = _case("levels_at_both_ends_in_mode_0_and_forward", [kf4()], [pt(102.5, V)], [0, 0], [[0, 0]] * 2, None,
              levels=[[0, 3]] * 2, modes=[0, 1])
    ends = {0: [1, 0], 1: [3, 2], 2: [3, 2, 1, 0], 3: [3]}
    _with(e, {i: (3 - a[0], 1) for i, a in ends.items()},
          lambda c, out: _assert(all(cands(c, i) == [3 - o for o in a] for i, a in ends.items())))
    return [c, e]


# ---- the radius and the stereo gate -------------------------------------------------------------------------------------

def radius_cases():
    """|dx| == r is outside and marked; one unit in the last place inside is a candidate (and marked as well); the same
    along y."""
    out = []
    for axis in (0, 1):
        on = (103.5, 100.0) if axis == 0 else (100.0, 103.25)
        inside = (math.nextafter(103.5, 0.0), 100.0) if axis == 0 else (100.0, math.nextafter(103.25, 0.0))
        a, b = KfBuilder(), KfBuilder()
        a.add(*on, D(9), cell=(6, 6))
        b.add(*inside, D(9), cell=(6, 6))
        c = _case(f"on_the_radius_along_{'xy'[axis]}", [a, b], [pt(U, V)], [0, 1], [[0], [0]], None, marked=[0, 1])
        out.append(_with(c, {1: (0, 1)}, lambda c, o: _assert(cands(c, 0) == [] and cands(c, 1) == [0])))
    return out


def stereo_cases():
    """ur = 68.5 and r = 3.  |ur - uR| == r keeps the feature and marks; half a pixel more leaves it out without a mark;
    uR == 0 and uR < 0 apply no gate."""
    kfs = [_one_feature(ur=x) for x in (71.5, 65.5, 72.0, 65.0, 0.0, -5.0)]
    c = _case("stereo_gate_at_and_beyond_the_radius", kfs, [pt(U, V)], list(range(6)), [[0]] * 6, None, marked=[0, 1])
    return [_with(c, {0: (0, 1), 1: (0, 1), 4: (0, 1), 5: (0, 1)},
                  lambda c, o: _assert(geom(c, 0)[1][2] == 68.5 and cands(c, 2, stereo_gate=False) == [0]
                                       and cands(c, 3, stereo_gate=False) == [0]))]


# ---- blocked ------------------------------------------------------------------------------------------------------------

def blocked_cases():
    """The best feature blocked: the next best wins.  All blocked: none.  A blocked feature exactly on the radius marks
    nothing, an open one there does."""
    def kf3():
        kf = KfBuilder()
        kf.add(100.0, 100.0, D(1))
        kf.add(101.0, 100.0, D(1, 2))
        kf.add(103.5, 100.0, D(1, 2, 3), cell=(6, 6))
        return kf
    c = _case("blocked_best_all_blocked_and_blocked_on_the_radius", [kf3(), kf3(), kf3(), kf3()], [pt(U, V)],
              [0, 1, 2, 3], [[0]] * 4, None, blocked=[[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 0, 0]], marked=[3])
    return [_with(c, {0: (0, 1), 1: (1, 2), 3: (0, 1)},
                  lambda c, o: _assert(cands(c, 1, blocked=False) == [0, 1] and cands(c, 2) == []))]


# ---- ties and the reduction ---------------------------------------------------------------------------------------------

def tie_cases():
    """Four features at the same distance in three cells of one window: column outer, row inner, then the cell's stored
    order.  Blocking the winner shows the next in line."""
    def kf():
        b = KfBuilder()
        b.add(113.0, 110.0, D(3))             # 0: cell (7, 6)
        b.add(110.0, 113.0, D(3))             # 1: cell (6, 7)
        b.add(110.0, 110.0, D(3))             # 2: cell (6, 6), stored first
        b.add(111.0, 111.0, D(3))             # 3: cell (6, 6), stored second
        return b
    blocked = [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1], [0, 1, 1, 1]]
    c = _case("ties_by_visiting_order", [kf() for _ in blocked], [pt(111.5, 111.5)], [0, 1, 2, 3], [[0]] * 4, None,
              blocked=blocked)
    return [_with(c, {0: (2, 1), 1: (3, 1), 2: (1, 1), 3: (0, 1)},
                  lambda c, o: _assert(cands(c, 0) == [2, 3, 1, 0]))]


def lane_cases():
    """17 entries in one column's range, so the 16-lane group goes round twice: the best is the 17th; and of two equal
    distances at entries 0 and 16 the first wins."""
    kf = KfBuilder()
    for j in range(17):
        kf.add(100.0, 100.0, D(*R(0, 18 - j)), cell=(6, 6))       # distances 18 ... 2
    one = _simple("window_17", kf, [pt(U, V)], {0: (16, 2)}, extra=lambda c, o: _assert(len(cands(c, 0)) == 17))
    kf = KfBuilder()
    for j in range(17):
        kf.add(100.0, 100.0, D(1) if j in (0, 16) else D(*R(0, 5 + j)), cell=(6, 6))
    return [one, _simple("window_17_tie_across_the_wrap", kf, [pt(U, V)], {0: (0, 1)})]


# ---- both eps -----------------------------------------------------------------------------------------------------------

def eps_cases():
    """A feature 2^-30 px inside the radius: unmarked under float64's eps, marked under float32's; the answer is the
    same."""
    out = []
    for eps, tag, marked in ((FO.EPS_F64, "f64", []), (FO.EPS_F32, "f32", [0])):
        kf = KfBuilder()
        kf.add(103.5 - 2.0 ** -30, 100.0, D(9), cell=(6, 6))
        out.append(_simple(f"just_inside_the_radius_eps_{tag}", kf, [pt(U, V)], {0: (0, 1)}, marked=marked, eps=eps))
    return out


def all_cases():
    out = [ragged_case([0, 1, 255, 256, 257], "ragged_0_1_255_256_257"), ragged_case([0], "zero_items"),
           ragged_case([], "zero_searches"), two_searches_case(), frames_case()]
    out += depth_cases() + [order_case()] + bound_cases() + window_cases() + octave_cases() + radius_cases()
    out += stereo_cases() + blocked_cases() + tie_cases() + lane_cases() + eps_cases()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


# ---- stand-ins and the golden -------------------------------------------------------------------------------------------

LEVELS = 8
N_PAIRS = 6
REDO_CAP = 0.05


class Frame(MF.GridFrame):
    """matcher_frames.GridFrame with what the array form of a frame reads besides (the level count and the log scale
    factor)."""

    def __init__(self, a, T, **kw):
        super().__init__(a, **kw)
        self.mnScaleLevels = LEVELS
        self.mfLogScaleFactor = math.log(1.2)
        self.mTcw = T


def complete(F):
    """A matcher_frames.GridFrame (matcher_ff_*.npz) with the two attributes above."""
    F.mnScaleLevels = LEVELS
    F.mfLogScaleFactor = math.log(1.2)
    return F


def load_pair(z, k):
    """(cur, last, mps, extra, th) of pair k of ff_many.npz, in matcher_frames.load_ff's layout under the prefix
    p<k>_."""
    q = {key[len(f"p{k}_"):]: z[key] for key in z.files if key.startswith(f"p{k}_")}
    cur = Frame({x[4:]: q[x] for x in q if x.startswith("cur_")}, q["Tc"])
    last = Frame({x[5:]: q[x] for x in q if x.startswith("last_")}, q["Tl"])
    mps = [MF.MP(q["mp_desc"][i], pos=q["mp_pos"][i].reshape(3, 1), obs=int(q["mp_obs"][i])) if q["mp_has"][i] else None
           for i in range(last.N)]
    last.mvpMapPoints = mps
    last.mvbOutlier = [bool(v) for v in q["mp_outlier"]]
    pre = q["pre"]
    extra = [None] * int((pre >= 0).sum())
    for j in np.nonzero(pre >= 0)[0]:
        extra[pre[j]] = MF.MP(cur.mDescriptors[j], pos=np.zeros((3, 1), np.float32), obs=int(q["pre_obs"][j]))
        cur.mvpMapPoints[j] = extra[pre[j]]
    return cur, last, mps, extra, float(q["th"])


def load_world(z):
    """Every pair of ff_many.npz, rebuilt: (jobs, per pair (mps, extra))."""
    pairs = [load_pair(z, k) for k in range(N_PAIRS)]
    return [(p[0], p[1], p[4]) for p in pairs], [(p[2], p[3]) for p in pairs]


def load_fixtures():
    """The six matcher_ff_*.npz pairs, completed: (jobs, per pair (mps, extra), per pair (n_matches, assigned))."""
    jobs, objs, want = [], [], []
    for case in range(6):
        cur, last, mps, extra, z = MF.load_ff(case)
        jobs.append((complete(cur), complete(last), float(z["th"])))
        objs.append((mps, extra))
        want.append((int(z["n_matches"]), z["assigned"]))
    return jobs, objs, want


def state(jobs, objs):
    """What a call leaves behind: per pair the current frame's slots in matcher_frames.encode_ff's code."""
    return [MF.encode_ff(cur, mps, extra) for (cur, _, _), (mps, extra) in zip(jobs, objs)]


def golden_results(z):
    return [int(z[f"p{k}_n_matches"]) for k in range(N_PAIRS)], [z[f"p{k}_assigned"] for k in range(N_PAIRS)]


def same(got, want):
    return list(got[0]) == list(want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
