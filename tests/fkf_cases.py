"""Cases for k_fkf_search on the geometry of tests/fuse_cases.py (identity pose, fx = fy = 64, cx = cy = 0, the image
[0, 640] x [0, 480], 16 px cells, four levels with the scale factors 1, 1.25, 1.5, 2; th = 3): a point made by
`pt(u, v)` lands on exactly (u, v) and every gate is decided by small dyadic numbers.  A search is a target frame and a
list of rows of one shared point table; a frame has one blocked byte per feature.  Each case carries its claim as a
`check` over the array oracle's flat results, which tests/test_fkf_cpu.py runs, so the GPU test that compares the
kernel with the oracle cannot pass on inputs that miss the situation.

A case: name, frames (fuse_oracle keyframe dicts), blocked (per frame, or None), pt_f64 / pt_desc (the point table),
srch_kf / items (per search its target and its rows of the table), th, eps, check(best_idx, best_dist, status) and
marked (the items built to come back ORBFE_FUSE_MARGINAL; no other item may).

Also the Frame stand-in with the reference's Frame surface, and the drivers of the golden tests/golden/fkf.npz, shared
by its generator and the tests.
"""
from __future__ import annotations

import numpy as np

import fkf_oracle as FK
import fuse_cases as FC
import fuse_oracle as O
import matcher_world as MW
from bow_match_cases import D, R
from fuse_cases import CELL, TH, KfBuilder, pt

CHUNK = FC.CHUNK
NAN = float("nan")
SCALE5 = [1.0, 1.25, 1.5, 2.0, 2.5]
SIG5 = [1.0, 0.5, 0.25, 0.125, 0.0625]


class Frame(MW.Frame):
    """matcher_world's Frame with the names the reference's Frame gives its grid size (Frame.py:373-416)."""

    def __init__(self, world, a, Tcw):
        super().__init__(world, a, Tcw)
        self.FRAME_GRID_COLS, self.FRAME_GRID_ROWS = self.mnGridCols, self.mnGridRows


def _case(name, frames, points, srch_kf, items, check, blocked=None, th=TH, eps=O.EPS_F64, marked=()):
    return dict(name=name, frames=[f.build() if isinstance(f, KfBuilder) else f for f in frames], blocked=blocked,
                pt_f64=np.array([p[0] for p in points], np.float64).reshape(-1, O.PT_F64),
                pt_desc=np.array([p[1] for p in points], np.uint8).reshape(-1, 32), srch_kf=list(srch_kf),
                items=[list(it) for it in items], th=th, eps=eps, check=check, marked=list(marked))


def _simple(name, kf, points, want, marked=(), status=None, **kw):
    """One search of every point into one frame; want: {item: (idx, dist)}."""
    def check(bi, bd, st):
        _expect(bi, bd, want)
        assert np.flatnonzero(st).tolist() == list(marked) if status is None else st.tolist() == status
    return _case(name, [kf], points, [0], [list(range(len(points)))], check, marked=marked, **kw)


def arrays(case):
    return FK.join(case["frames"], case["blocked"], case["pt_f64"], case["pt_desc"], case["srch_kf"], case["items"],
                   case["th"], case["eps"])


def oracle(case, **kw):
    return FK.search(arrays(case), **kw)


def geom(case, i, **kw):
    """The oracle's phase 1 of item i: (status, window or None)."""
    a = arrays(case)
    return FK._window(a, FK.search_of(a, i), i, **kw)[2]


def _expect(bi, bd, want):
    """want: {item: (idx, dist)}; every other item has no candidate."""
    assert bi.ndim == 1 and bi.shape == bd.shape
    for i in range(len(bi)):
        assert (int(bi[i]), int(bd[i])) == want.get(i, (-1, -1)), (i, bi[i], bd[i])


def _one_feature():
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9))
    return kf


def _with(case, check):
    case["check"] = check
    return case


# ---- the launch shape -------------------------------------------------------------------------------------------------

def _table():
    """A lattice frame of 20 features and a table of 80 points: row j looks at feature j % 20 from 3 + j // 20 bits
    away."""
    kf = FC._lattice_kf(20)
    pts = [pt(50.5 + 40.0 * (j % 20 % 12), 60.25 + 40.0 * (j % 20 // 12), desc=D(*R(200, 200 + j // 20)))
           for j in range(80)]
    return kf, pts


def ragged_case(sizes, name):
    """Searches of the given item counts over one table; search s starts at row 7 s and walks the table with stride
    3, so the chunks of different searches hold different rows."""
    kf, pts = _table()
    items = [[(7 * s + 3 * c) % 80 for c in range(n)] for s, n in enumerate(sizes)]
    want, i = {}, 0
    for it in items:
        for r in it:
            want[i] = (r % 20, 3 + r // 20)
            i += 1

    def check(bi, bd, st):
        assert len(bi) == sum(sizes)
        _expect(bi, bd, want)
        assert not st.any()
    return _case(name, [kf], pts, [0] * len(sizes), items, check)


def frames_case():
    """Four frames in one launch: the standard one; one with 32 px cells on a 20 x 15 grid, five levels and a pose
    moved a quarter of a unit along x (16 px); one without features; and one that no search targets.  The same point
    is looked for in the first three; a second point of level 4 exists only in the second frame's level table."""
    a = KfBuilder()
    a.add(100.0, 100.0, D(1))
    a.add(116.0, 100.0, D(1, 2))
    b = KfBuilder(cols=20, rows=15, inv=(1.0 / 32, 1.0 / 32), scale=SCALE5, inv_sigma2=SIG5, t=(0.25, 0.0, 0.0),
                  Ow=(-0.25, 0.0, 0.0))
    b.add(100.0, 100.0, D(1), cell=(3, 3))
    b.add(116.0, 100.0, D(1, 2), cell=(3, 3))
    b.add(300.0, 200.0, D(1, 2, 3), octave=4, cell=(9, 6))
    far = pt(300.5 - 16.0, 200.25, q=3.9)
    c = _case("four_frames_two_grids_one_empty_one_idle", [a, b, KfBuilder(), _one_feature()],
              [pt(100.5, 100.25), far], [0, 1, 2], [[0], [0, 1], [0]], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {0: (0, 1), 1: (1, 2), 2: (2, 3)})
        assert geom(c, 1)[1][0] == 116.5 and geom(c, 2)[1][5] == 4
        assert 3 not in c["srch_kf"] and len(c["frames"][2]["xy"]) == 0 and not st.any()
    return _with(c, check)


# ---- the depth ------------------------------------------------------------------------------------------------------

def behind_case():
    """A point behind the camera (z = -1) that projects to the pixel its mirror image does, and finds the feature:
    a depth gate would skip it.  z == 0 is marked, whatever x is."""
    front = pt(100.5, 100.25)
    behind = ([-front[0][0], -front[0][1], -1.0] + front[0][3:], D())
    flat0 = (front[0][:2] + [0.0] + front[0][3:], D())
    flat1 = ([0.0, 0.0, 0.0] + front[0][3:], D())
    c = _simple("behind_the_camera_is_searched_and_depth_zero_marked", _one_feature(), [behind, flat0, flat1, front],
                {0: (0, 1), 3: (0, 1)}, marked=[1, 2])
    inner = c["check"]

    def check(bi, bd, st, c=c):
        inner(bi, bd, st)
        assert c["pt_f64"][0][2] < 0 and geom(c, 0)[1][:2] == (100.5, 100.25)
        assert geom(c, 0, depth_gate=True)[1] is None
        assert c["pt_f64"][1][2] == 0.0 == c["pt_f64"][2][2]
    return _with(c, check)


# ---- the image bounds -------------------------------------------------------------------------------------------------

def bound_cases():
    """u exactly on mnMaxX and v exactly on mnMinY (16 here, so that the bound is not zero): inside, since both ends
    are inclusive, and marked, since u and v are rounded quantities.  u 60 px outside: skipped, unmarked."""
    kf = KfBuilder()
    kf.add(639.0, 100.0, D(9), cell=(39, 6))
    at_max = _simple("u_on_max_x_is_inside_and_marked", kf, [pt(640.0, 100.25), pt(700.5, 100.25)], {0: (0, 1)},
                     marked=[0])
    inner = at_max["check"]

    def check(bi, bd, st, c=at_max):
        inner(bi, bd, st)
        assert geom(c, 0)[1][0] == 640.0 == c["frames"][0]["f64"][21]
        assert geom(c, 0, exclusive_max=True)[1] is None and geom(c, 1) == (0, None)
    _with(at_max, check)
    kf = KfBuilder(bounds=(0.0, 640.0, 16.0, 480.0))
    kf.add(100.0, 17.0, D(9), cell=(6, 0))
    at_min = _simple("v_on_min_y_is_inside_and_marked", kf, [pt(100.5, 16.0)], {0: (0, 1)}, marked=[0])
    inner2 = at_min["check"]

    def check2(bi, bd, st, c=at_min):
        inner2(bi, bd, st)
        assert geom(c, 0)[1][1] == 16.0 == c["frames"][0]["f64"][22]
    _with(at_min, check2)
    return [at_max, at_min]


# ---- the distance -----------------------------------------------------------------------------------------------------

def distance_case():
    """|p - Ow| exactly on the minimum and on the maximum invariance distance: both pass and both are marked.  A
    thousandth inside: unmarked and found.  A thousandth outside: skipped, unmarked."""
    pts = [pt(100.5, 100.25, min_f=1.0), pt(100.5, 100.25, max_f=1.0), pt(100.5, 100.25, min_f=0.999),
           pt(100.5, 100.25, max_f=1.001), pt(100.5, 100.25, min_f=1.001), pt(100.5, 100.25, max_f=0.999)]
    c = _simple("distance_on_min_and_max_marked_outside_skipped", _one_feature(), pts,
                {i: (0, 1) for i in range(4)}, marked=[0, 1])
    inner = c["check"]

    def check(bi, bd, st, c=c):
        inner(bi, bd, st)
        assert geom(c, 4) == (0, None) and geom(c, 5) == (0, None)
    return _with(c, check)


def normal_case():
    """NaN in the normal's slots, which the kernel does not read: found, where a viewing gate finds nothing."""
    p = pt(100.5, 100.25)
    c = _simple("normal_slots_hold_nan_and_no_viewing_gate", _one_feature(), [(p[0][:3] + [NAN] * 3 + p[0][6:], p[1])],
                {0: (0, 1)})
    inner = c["check"]

    def check(bi, bd, st, c=c):
        inner(bi, bd, st)
        assert np.isnan(c["pt_f64"][0][3:6]).all() and geom(c, 0, viewing_gate=True)[1] is None
    return _with(c, check)


# ---- levels and octaves -----------------------------------------------------------------------------------------------

def level_case():
    """Quotients -2.5 and 7.5 clamp to levels 0 and 3; the features' octaves (0 and 3) tell which level was used."""
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9), octave=0)
    kf.add(101.0, 100.0, D(9, 10), octave=3)
    c = _simple("level_clamped_low_and_high", kf, [pt(100.5, 100.25, q=-2.5), pt(100.5, 100.25, q=7.5)],
                {0: (0, 1), 1: (1, 2)})
    inner = c["check"]

    def check(bi, bd, st, c=c):
        inner(bi, bd, st)
        assert geom(c, 0)[1][5] == 0 and geom(c, 1)[1][5] == 3
    return _with(c, check)


def octave_cases():
    """Level 1 and the closest descriptor at octave 2: it wins, where two octaves would take the one at octave 1.
    Level 2 of five: octaves 0 and 4 hold closer descriptors and are left out."""
    kf = KfBuilder()
    kf.add(101.0, 100.0, D(1), octave=2)
    kf.add(101.0, 101.0, D(1, 2, 3), octave=1)
    up = _simple("octave_one_above_the_level_wins", kf, [pt(101.5, 100.25, level=1)], {0: (0, 1)})
    inner = up["check"]

    def check(bi, bd, st, c=up):
        inner(bi, bd, st)
        got = oracle(c, two_octaves=True)
        assert (int(got[0][0]), int(got[1][0])) == (1, 3)
    _with(up, check)
    kf = KfBuilder(scale=SCALE5, inv_sigma2=SIG5)
    kf.add(101.0, 100.0, D(1), octave=0)
    kf.add(101.0, 101.0, D(1, 2), octave=4)
    kf.add(102.0, 100.0, D(1, 2, 3, 4), octave=3)
    kf.add(102.0, 101.0, D(1, 2, 3, 4, 5), octave=1)
    out = _simple("octaves_two_away_are_left_out", kf, [pt(101.5, 100.25, level=2)], {0: (2, 4)})
    return [up, out]


# ---- blocked, ties, the radius, the window ------------------------------------------------------------------------------

def blocked_cases():
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1))
    kf.add(101.0, 100.0, D(1, 2, 3))
    one = _simple("closest_candidate_blocked", kf, [pt(100.5, 100.25)], {0: (1, 3)}, blocked=[[1, 0]])
    inner = one["check"]

    def check(bi, bd, st, c=one):
        inner(bi, bd, st)
        got = oracle(c, blocked=False)
        assert (int(got[0][0]), int(got[1][0])) == (0, 1)
    _with(one, check)
    # a blocked entry marks nothing either: the second feature lies exactly one radius away
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1))
    kf.add(103.5, 100.0, D(1, 2))
    every = _simple("every_candidate_blocked", kf, [pt(100.5, 100.25)], {}, blocked=[[1, 1]])
    inner2 = every["check"]

    def check2(bi, bd, st, c=every):
        inner2(bi, bd, st)
        assert oracle(c, blocked=False)[2].tolist() == [O.MARGINAL]
    _with(every, check2)
    return [one, every]


def tie_cases():
    kf = KfBuilder()
    kf.add(112.5, 100.0, D(1, 2))   # index 0 in column 7: visited after column 6
    kf.add(111.5, 100.0, D(3, 4))   # index 1 in column 6
    two = _simple("tie_in_two_cells", kf, [pt(112.0, 100.25)], {0: (1, 2)})
    kf = KfBuilder()
    for j, d in enumerate((D(1, 2), D(1, 2, 3), D(3, 4))):
        kf.add(100.0 + j, 100.0, d, cell=None)
    kf.cells[(6, 6)] = [2, 1, 0]    # stored order: 2 first, though 0 has the same distance
    one = _simple("tie_in_one_unsorted_cell", kf, [pt(100.5, 100.25)], {0: (2, 2)})
    return [two, one]


def radius_case():
    """r = 3: the closer descriptor is 3.25 px away, the other 2.75 px."""
    kf = KfBuilder()
    kf.add(103.75, 100.25, D(1), cell=(6, 6))
    kf.add(103.25, 100.25, D(1, 2, 3), cell=(6, 6))
    return _simple("feature_just_inside_and_just_outside_the_radius", kf, [pt(100.5, 100.25)], {0: (1, 3)})


def window_cases():
    """Both ends truncate.  The upper end: (100.5 + 3) / 16 = 6.47 is column 6, and a feature stored in column 7 is
    not visited, which a ceil would.  The clamp at the last column.  The four early returns: a grid of 10 x 10 cells
    in the same image, and th = -20, whose upper end is at most -1."""
    kf = KfBuilder()
    kf.add(101.0, 100.0, D(1), cell=(7, 6))
    kf.add(100.0, 100.0, D(1, 2, 3), cell=(6, 6))
    out = [_simple("upper_end_truncates", kf, [pt(100.5, 100.25)], {0: (1, 3)})]
    inner = out[0]["check"]

    def check(bi, bd, st, c=out[0]):
        inner(bi, bd, st)
        assert geom(c, 0)[1][6:8] == (6, 6) and geom(c, 0, floor_ceil=True)[1][6:8] == (6, 7)
    _with(out[0], check)
    kf = KfBuilder()
    kf.add(637.0, 100.0, D(9))
    last = _simple("clamp_col_last", kf, [pt(638.5, 100.25)], {0: (0, 1)})
    inner_l = last["check"]

    def check_l(bi, bd, st, c=last):
        inner_l(bi, bd, st)
        assert geom(c, 0)[1][7] == FC.COLS - 1 < int((638.5 + TH) / CELL)
    out.append(_with(last, check_l))
    for name, (u, v), th in (("x0", (300.5, 100.25), TH), ("x1", (1.5, 100.25), -20.0), ("y0", (100.5, 300.25), TH),
                             ("y1", (100.5, 1.25), -20.0)):
        kf = KfBuilder(cols=10, rows=10)
        kf.add(100.0, 100.0, D(9))
        kf.add(2.0, 100.0, D(9))
        kf.add(100.0, 2.0, D(9))
        c = _simple(f"early_return_{name}", kf, [pt(u, v)], {}, th=th)
        inner_e = c["check"]

        def check_e(bi, bd, st, c=c, name=name, u=u, v=v, th=th, inner_e=inner_e):
            inner_e(bi, bd, st)
            assert geom(c, 0) == (0, None)
            raw = dict(x0=int((u - th) / CELL) >= 10, x1=int((u + th) / CELL) < 0,
                       y0=int((v - th) / CELL) >= 10, y1=int((v + th) / CELL) < 0)
            assert [k for k, hit in raw.items() if hit] == [name]
        out.append(_with(c, check_e))
    return out


def many_candidates():
    """65 candidates in a level-3 window (radius 6) over the cells of one column: more than four rounds of the 16
    lanes; the best descriptor is the last visited."""
    c0 = FC.window_case(65)
    c = _case("window_65", c0["frames"], list(zip(c0["pt_f64"].tolist(), c0["pt_desc"])), [0], [[0, 1]], None)

    def check(bi, bd, st):
        _expect(bi, bd, {0: (64, 2), 1: (65 // 3, 9)})
    return _with(c, check)


def eps_cases():
    out = []
    for name, eps in (("eps_of_float32", O.EPS_F32), ("eps_of_float64", O.EPS_F64)):
        kf = KfBuilder()
        kf.add(100.0, 100.0, D(1, 2, 3))
        c = _simple(name, kf, [pt(100.5, 100.25)], {0: (0, 3)}, eps=eps)
        out.append(c)
    # a feature 2^-30 of a pixel inside the radius: float32's unit of rounding marks it, float64's does not
    kf = KfBuilder()
    kf.add(103.5 - 2.0 ** -30, 100.25, D(1), cell=(6, 6))
    out.append(_simple("eps_of_float32_marks_what_float64_does_not", kf, [pt(100.5, 100.25)], {0: (0, 1)}, marked=[0],
                       eps=O.EPS_F32))
    out.append(_simple("eps_of_float64_leaves_it_unmarked", kf, [pt(100.5, 100.25)], {0: (0, 1)}, eps=O.EPS_F64))
    return out


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = ([ragged_case((1, 0, 255, 256, 0, 257, 0), "ragged_0_1_255_256_257"), ragged_case((0, 0), "zero_items"),
                 ragged_case((), "zero_searches"), frames_case(), behind_case()] + bound_cases()
                + [distance_case(), normal_case(), level_case()] + octave_cases() + blocked_cases() + tie_cases()
                + [radius_case()] + window_cases() + [many_candidates()] + eps_cases())
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


# ---- search_by_projection_f_kf_f on a matcher_world world (shared by the golden's generator and the tests) ----------

N_SEARCH = 6
FRAME_KF = 6                                  # the keyframe of the clone_world whose arrays and pose make the frame
CONFIGS = ((10.0, 100, True), (3.0, 64, True), (10.0, 100, False), (3.0, 64, False))   # th, ORBdist, orientation


def make_extras(z, seed, n_behind=8, n_twins=6):
    """What the golden adds to a fuse_cases.clone_world (changed in place): fkf_T, the frame's pose (keyframe 6's,
    moved a little); fkf_pre, the frame's slots before a call (about a quarter filled: the map point the feature
    re-observes where there is one, else any); fkf_found{k}, the map points of search k's sAlreadyFound (a tenth of
    keyframe k's, never empty); and n_behind map points of keyframes 0..5 mirrored through the frame's camera centre,
    which project where they did, from behind."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = z[f"kf{FRAME_KF}_T"].copy()
    T[:3, 3] += rng.normal(0, 0.02, 3).astype(np.float32)
    z["fkf_T"] = T
    n = len(z[f"kf{FRAME_KF}_x"])
    n_mp = len(z["mp_desc"])
    slots = z[f"kfmp{FRAME_KF}"]
    pre = np.full(n, -1, np.int32)
    for i in rng.choice(n, n // 4, replace=False).tolist():
        pre[i] = slots[i] if slots[i] >= 0 else int(rng.integers(n_mp))
    z["fkf_pre"] = pre
    held = [np.unique(z[f"kfmp{k}"][z[f"kfmp{k}"] >= 0]) for k in range(N_SEARCH)]
    for k in range(N_SEARCH):
        z[f"fkf_found{k}"] = rng.choice(held[k], max(1, len(held[k]) // 10), replace=False).astype(np.int32)
    R_, t_ = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    Ow = -R_.T @ t_
    pool = np.unique(np.concatenate(held))
    pos = z["mp_pos"].copy()
    for m in rng.choice(pool, n_behind, replace=False).tolist():
        pos[m] = (2.0 * Ow - pos[m].astype(np.float64)).astype(np.float32)
    z["mp_pos"] = pos
    z["fkf_behind"] = np.int32(n_behind)
    # twins: in every keyframe a few free slots get a new map point next to one the keyframe holds already (nearly
    # the same position, a descriptor a few bits away), so two items of one search want the same feature
    new = {key: [] for key in ("mp_pos", "mp_normal", "mp_desc", "mp_min", "mp_max", "mp_bad")}
    for k in range(N_SEARCH):
        slots_k = z[f"kfmp{k}"]
        free = np.flatnonzero(slots_k < 0)
        for i, m in zip(rng.choice(free, n_twins, replace=False).tolist(),
                        rng.choice(held[k], n_twins, replace=False).tolist()):
            slots_k[i] = n_mp + len(new["mp_bad"])
            new["mp_pos"].append(z["mp_pos"][m] + rng.normal(0, 0.002, 3).astype(np.float32))
            new["mp_desc"].append(MW.noisy_desc(rng, z["mp_desc"][m], int(rng.integers(0, 6))))
            new["mp_bad"].append(False)
            for key in ("mp_normal", "mp_min", "mp_max"):
                new[key].append(z[key][m])
    for key, rows in new.items():
        z[key] = np.concatenate([z[key], np.array(rows, z[key].dtype).reshape((-1,) + z[key].shape[1:])])
    return z


def jobs_of(w, g):
    """[(frame copy k, keyframe k, sAlreadyFound k)] of a fresh world: every search has a frame object of its own."""
    a = MW.sub(g, f"kf{FRAME_KF}_")
    jobs = []
    for k in range(N_SEARCH):
        F = Frame(w, a, g["fkf_T"])
        F.mvpMapPoints = [w.mps[int(m)] if m >= 0 else None for m in g["fkf_pre"]]
        jobs.append((F, w.kfs[k], {w.mps[int(m)] for m in g[f"fkf_found{k}"]}))
    return jobs


def drive(g, run, cfg):
    """The six searches of a configuration on a fresh world through run(jobs, th, orb_dist, orientation) -> [n]:
    (the ns, the encoded slots of every frame afterwards)."""
    w = MW.build(g)
    jobs = jobs_of(w, g)
    ns = run(jobs, *CONFIGS[cfg])
    return [int(n) for n in ns], np.stack([MW.encode_mps(w, j[0].mvpMapPoints) for j in jobs])


def loop_single(matcher_cls, method="search_by_projection_f_kf_f"):
    def run(jobs, th, orb, ori):
        m = matcher_cls(1, ori)
        return [getattr(m, method)(F, kf, found, th, orb) for F, kf, found in jobs]
    return run


def many(matcher_cls):
    def run(jobs, th, orb, ori):
        return matcher_cls(1, ori).search_by_projection_f_kf_f_many(*[[j[c] for j in jobs] for c in range(3)], th, orb)
    return run


def by_oracle(stats=None, agree=False, results=None):
    def run(jobs, th, orb, ori):
        return FK.replay(jobs, th, orb, ori, results=results, stats=stats, agree=agree)
    return run


def golden_results(g, cfg):
    return [int(n) for n in g[f"fkf_n{cfg}"]], g[f"fkf_slots{cfg}"]


def same(got, want):
    return got[0] == want[0] and np.array_equal(got[1], want[1])
