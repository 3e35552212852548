"""Cases for k_scw_search on the geometry of tests/fuse_cases.py (identity pose, fx = fy = 64, 16 px cells, four levels
with the scale factors 1, 1.25, 1.5, 2; th = 3 unless a case says otherwise).  The cases of k_fuse_search that do not
hinge on the chi-square are taken over as they are; those that exist for what k_scw_search changes are made here:
the depth gate at and around zero, candidates the chi-square would refuse, the blocked byte, poses from a Sim3.  Each
case carries its claim as a `check` over the array oracle's results, which tests/test_scw_cpu.py runs, so the GPU
test that compares the kernel with the oracle cannot pass on inputs that miss the situation.

A case: name, frames (fuse_oracle keyframe dicts), blocked (None, or one list of bytes per keyframe), pt_f64 /
pt_desc, th, eps, check(best_idx, best_dist, status) and marginal (True for the one case built to be marked).

Also the drivers of the golden tests/golden/scw_many.npz, shared by its generator and the tests.
"""
from __future__ import annotations

import math

import numpy as np

import fuse_cases as FC
import fuse_oracle as O
import scw_oracle as SO
from bow_match_cases import D, R
from fuse_cases import BF, CELL, COLS, ROWS, TH, KfBuilder, _expect, pt

CHUNK, GROUP = FC.CHUNK, FC.GROUP


def _case(name, frames, points, check, th=TH, eps=O.EPS_F64, marginal=False, blocked=None):
    c = FC._case(name, frames, points, check, th=th, eps=eps, marginal=marginal)
    c["blocked"] = blocked
    return c


def taken_over(c):
    c = dict(c)
    c["blocked"] = None
    return c


def arrays(case):
    blk = case["blocked"]
    if blk is not None:
        blk = np.concatenate([np.asarray(b, np.uint8) for b in blk]) if blk else np.zeros(0, np.uint8)
    return SO.from_fuse(FC.arrays(case), blk)


def oracle(case, **kw):
    return SO.search(arrays(case), **kw)


def geom(case, k, i):
    f = case["frames"][k]
    return SO.geometry(f["f64"], f["i32"], f["scale"], case["pt_f64"][i], case["th"], case["eps"])


# ---- the depth gate ---------------------------------------------------------------------------------------------

def depth_cases():
    """z == 0 twice (u inf, u NaN), z = -2^-20 and z = +2^-20 at the same pixel: only the last finds the feature."""
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9))
    ref = pt(100.5, 100.25)[0]
    flat0 = (ref[:2] + [0.0] + ref[3:], D())           # z == 0, x != 0: u is inf
    flat1 = ([0.0, 0.0, 0.0] + ref[3:], D())           # z == 0, x == 0: u is NaN
    z = 2.0 ** -20
    behind = pt(100.5, 100.25, z=z)
    behind[0][0:3] = [-c for c in behind[0][0:3]]      # the same pixel from just behind the camera
    c = _case("depth_zero_and_either_side", [kf], [flat0, flat1, behind, pt(100.5, 100.25, z=z)], None)

    def check(bi, bd, st, c=c, z=z):
        _expect(bi, bd, {(0, 3): (0, 1)})
        assert [float(r[2]) for r in c["pt_f64"]] == [0.0, 0.0, -z, z]
        assert not st.any()
    c["check"] = check
    return [c]


# ---- no chi-square ------------------------------------------------------------------------------------------------

def chi_cases():
    """The geometry of fuse_cases.chi_cases: inside the radius of 3 px, a squared error of 6.25 (mono, above 5.99)
    and of 9 (stereo, above 7.8) with the closer descriptor.  k_fuse_search refuses that feature; here it wins."""
    out = []
    for c0 in FC.chi_cases():
        c = taken_over(c0)
        c["name"] = c0["name"].replace("chi_square", "no_chi_square")

        def check(bi, bd, st, c0=c0):
            _expect(bi, bd, {(0, 0): (0, 1)})
            fbi, fbd, _ = FC.oracle(c0)
            assert (int(fbi[0, 0]), int(fbd[0, 0])) == (1, 3)   # what a chi gate left in would give
            f = c0["frames"][0]
            u, v = 100.5, 100.25
            e2 = (u - f["xy"][0][0]) ** 2 + (v - f["xy"][0][1]) ** 2
            if f["u_right"][0] >= 0:
                assert e2 + ((u - BF) - f["u_right"][0]) ** 2 > 7.8
            else:
                assert e2 > 5.99
        c["check"] = check
        out.append(c)
    return out


# ---- the blocked byte -----------------------------------------------------------------------------------------------

def _three():
    """Three features around (100.5, 100.25) in one cell: distances 1, 2 and 2, stored in that order."""
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1), cell=(6, 6))
    kf.add(101.0, 100.0, D(1, 2), cell=(6, 6))
    kf.add(101.0, 101.0, D(3, 4), cell=(6, 6))
    return kf


def blocked_cases():
    p = [pt(100.5, 100.25)]
    return [
        _case("blocked_nearest_gives_the_next", [_three()], p, lambda bi, bd, st: _expect(bi, bd, {(0, 0): (1, 2)}),
              blocked=[[1, 0, 0]]),
        _case("blocked_all_gives_none", [_three()], p, lambda bi, bd, st: _expect(bi, bd, {}), blocked=[[1, 1, 1]]),
        _case("blocked_earlier_of_a_tie_gives_the_later", [_three()], p,
              lambda bi, bd, st: _expect(bi, bd, {(0, 0): (2, 2)}), blocked=[[1, 1, 0]]),
        _case("blocked_null_mask", [_three()], p, lambda bi, bd, st: _expect(bi, bd, {(0, 0): (0, 1)})),
        _case("blocked_other_values_than_one", [_three()], p, lambda bi, bd, st: _expect(bi, bd, {(0, 0): (2, 2)}),
              blocked=[[255, 2, 0]]),
    ]


def blocked_ragged():
    """Two keyframes of different lengths: the bytes are read at each keyframe's own offset."""
    a, b = FC._lattice_kf(4), FC._lattice_kf(7)
    pts = [pt(50.5 + 40.0 * j, 60.25, desc=D(255)) for j in range(7)]
    want = {(0, 0): (0, 4), (0, 2): (2, 4), (1, 0): (0, 4), (1, 3): (3, 4), (1, 4): (4, 4), (1, 6): (6, 4)}
    return _case("blocked_ragged", [a, b], pts, lambda bi, bd, st: _expect(bi, bd, want),
                 blocked=[[0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 0]])


def blocked_marks_nothing():
    """A blocked feature exactly at the radius: unblocked it marks the item, blocked it decides nothing."""
    def kf():
        k = KfBuilder()
        k.add(103.5, 100.0, D(1), cell=(6, 6))
        k.add(100.0, 100.0, D(1, 2), cell=(6, 6))
        return k

    def check(bi, bd, st):
        _expect(bi, bd, {(0, 0): (1, 2)})
        assert not st.any()
    return _case("blocked_at_the_radius_marks_nothing", [kf()], [pt(100.5, 100.0)], check, blocked=[[1, 0]])


# ---- poses from a Sim3 ------------------------------------------------------------------------------------------------

def _scw(t, s):
    S = np.eye(4)
    S[:3, :3] *= s
    S[:3, 3] = [s * c for c in t]
    return S


def _posed(kf, S):
    return SO.with_pose(kf.build(), SO.fuse_pose(S))


def two_poses():
    """The same two features and the same point in two keyframes whose Scw differ by a quarter of a unit along x,
    16 px in the image: each keyframe finds the feature under its own projection."""
    def kf():
        k = KfBuilder()
        k.add(100.0, 100.0, D(1))
        k.add(116.0, 100.0, D(1, 2))
        return k
    frames = [_posed(kf(), _scw((0.0, 0.0, 0.0), 1.0)), _posed(kf(), _scw((0.25, 0.0, 0.0), 1.0))]
    c = _case("two_keyframes_two_poses", frames, [pt(100.5, 100.25)], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {(0, 0): (0, 1), (1, 0): (1, 2)})
        assert geom(c, 0, 0)[1][0] == 100.5 and geom(c, 1, 0)[1][0] == 116.5
    c["check"] = check
    return c


def sim3_scales():
    """One pose as a Sim3 of scale 1, 0.8 and 2: dividing the scale out gives the same projection."""
    def kf():
        k = KfBuilder()
        k.add(100.0, 100.0, D(1))
        k.add(116.0, 100.0, D(1, 2))
        return k
    frames = [_posed(kf(), _scw((0.25, 0.0, 0.0), s)) for s in (1.0, 0.8, 2.0)]
    c = _case("sim3_scales", frames, [pt(100.5, 100.25), pt(84.5, 100.25)], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {(k, i): w for k in range(3) for i, w in enumerate(((1, 2), (0, 1)))})
        for k in range(3):
            assert abs(geom(c, k, 0)[1][0] - 116.5) < 1e-9
        assert not st.any()
    c["check"] = check
    return c


# ---- the window at th = 10 ------------------------------------------------------------------------------------------

def clamp_cases():
    out = []
    th = 10.0
    for name, (u, v), (fx_, fy_), edge in (("col_0", (1.5, 100.25), (9.0, 100.0), (0, None)),
                                           ("col_last", (638.5, 100.25), (630.0, 100.0), (1, COLS - 1)),
                                           ("row_0", (100.5, 1.25), (100.0, 9.0), (2, None)),
                                           ("row_last", (100.5, 478.25), (100.0, 470.0), (3, ROWS - 1))):
        kf = KfBuilder()
        kf.add(fx_, fy_, D(9))
        c = _case(f"clamp_th10_{name}", [kf], [pt(u, v)], None, th=th)

        def check(bi, bd, st, c=c, edge=edge, u=u, v=v):
            _expect(bi, bd, {(0, 0): (0, 1)})
            w = geom(c, 0, 0)[1]
            raw = [math.floor((u - th) / CELL), math.ceil((u + th) / CELL), math.floor((v - th) / CELL),
                   math.ceil((v + th) / CELL)]
            lim = (0, COLS - 1, 0, ROWS - 1)
            assert w[6 + edge[0]] == lim[edge[0]] != raw[edge[0]]  # the clamp acted
        c["check"] = check
        out.append(c)
    return out


# ---- the marginal bit ----------------------------------------------------------------------------------------------

def marginal_case():
    """A feature exactly one radius (3 px) from the second point's projection: |dx| == r is no candidate, and within
    rounding of being one."""
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1), cell=(6, 6))
    kf.add(303.5, 100.0, D(1), cell=(18, 6))
    kf.add(300.0, 100.0, D(1, 2), cell=(18, 6))
    kf.add(500.0, 100.0, D(1), cell=(31, 6))
    pts = [pt(100.5, 100.0), pt(300.5, 100.0), pt(500.25, 100.0)]

    def check(bi, bd, st):
        _expect(bi, bd, {(0, 0): (0, 1), (0, 1): (2, 2), (0, 2): (3, 1)})
        assert st.tolist() == [[0, O.MARGINAL, 0]]
    return _case("marginal", [kf], pts, check, marginal=True)


def eps_f32_case():
    c = taken_over(FC.one_one())
    c.update(name="eps_of_float32", eps=O.EPS_F32)
    return c


# ---- keyframes with real poses, in both dtypes ---------------------------------------------------------------------

def pose_case(dtype, th=4.0):
    """A small matcher_world world with poses, positions and Scw of `dtype`; Scw = the keyframe's pose times 1.1 and
    0.9.  Unmarked items decide as the reference's loop body does."""
    import matcher_world as MW
    w = FC.pose_world(dtype)
    pts = [p for p in w.mps if not p.is_bad()]
    kfs = w.kfs[1:]
    Scws = [MW.sim3(kf.Tcw, s).astype(dtype) for kf, s in zip(kfs, (1.1, 0.9))]
    a = SO.pack(kfs, Scws, pts, th)
    frames = [SO.with_pose(O.pack_kf(kf), SO.fuse_pose(S)) for kf, S in zip(kfs, Scws)]
    c = dict(name=f"poses_{np.dtype(dtype).name}", frames=frames, blocked=None, pt_f64=a["pt_f64"],
             pt_desc=a["pt_desc"], th=th, eps=a["eps"], marginal=False)

    def check(bi, bd, st, c=c, dtype=dtype):
        assert c["eps"] == (O.EPS_F32 if dtype == np.float32 else O.EPS_F64)
        found = 0
        for k, (kf, S) in enumerate(zip(kfs, Scws)):
            pose = SO.fuse_pose(S)
            for i, p in enumerate(pts):
                if st[k, i]:
                    continue
                dist, idx = SO.single_item(kf, p, pose, th)
                assert (idx, dist if idx >= 0 else -1) == (int(bi[k, i]), int(bd[k, i])), (k, i)
                found += idx >= 0
        assert found > 10
    c["check"] = check
    return c


_ALL = None
# fuse_cases' own that hinge on the chi-square or the right coordinate, or that are restated here
_LEFT_OUT = ("chi_square_mono", "chi_square_stereo", "u_right_zero_is_stereo", "marginal", "eps_of_float32",
             "poses_float32", "poses_float64")


def all_cases():
    global _ALL
    if _ALL is None:
        kept = [taken_over(c) for c in FC.all_cases() if c["name"] not in _LEFT_OUT]
        _ALL = (kept + [taken_over(FC.chunk_case(2 * CHUNK + 1))] + [taken_over(FC.window_case(L)) for L in (15, 16, 17)]
                + depth_cases() + chi_cases() + blocked_cases() + [blocked_ragged(), blocked_marks_nothing(), two_poses(),
                                                                  sim3_scales()]
                + clamp_cases() + [marginal_case(), eps_f32_case()] + [pose_case(np.float32), pose_case(np.float64)])
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


# ---- LoopClosing's two searches on a matcher_world world (shared by the golden's generator and the tests) ----------

N_KFS = (1, 3, 6)
SCALES = (1.0, 1.1, 0.9)
TH_FUSE, TH_CKF = 4.0, 10.0
STATE = ("ret", "rep", "log", "slots", "bad", "desc")


def loop_points(w):
    """mvpLoopMapPoints: keyframe 0's map points, bad ones included (the searches skip them themselves)."""
    return [p for p in w.kfs[0].get_map_point_matches() if p is not None]


def replacer(points):
    """The replace loop of LoopClosing.search_and_fuse (LoopClosing.py:361-367)."""
    def replace(pKF, vpReplacePoints):
        for pRep, pLoop in zip(vpReplacePoints, points):
            if pRep:
                pRep.replace(pLoop)
    return replace


def scws(g, n):
    return [g[f"Scw{j}"] for j in range(1, n + 1)]


def drive_fuse(w, g, fuse_many, n, after=True):
    """search_and_fuse over keyframes 1..n of the world: fuse_many(kfs, Scws, points, th, after) returns the list of
    (nFused, vpReplacePoint)."""
    pts = loop_points(w)
    return fuse_many(w.kfs[1:1 + n], scws(g, n), pts, TH_FUSE, replacer(pts) if after else None)


def loop_fuse(single):
    """fuse_many as the loop of single(kf, Scw, points, th, vpReplacePoint) calls."""
    def fuse_many(kfs, Scws, pts, th, after):
        out = []
        for kf, S in zip(kfs, Scws):
            r = single(kf, S, pts, th, [None] * len(pts))
            if after is not None:
                after(kf, r[1])
            out.append(r)
        return out
    return fuse_many


def fuse_state(w, res):
    import matcher_world as MW
    P = len(res[0][1]) if res else 0
    return dict(ret=np.array([r[0] for r in res], np.int32),
                rep=np.array([MW.encode_mps(w, r[1]) for r in res], np.int32).reshape(len(res), P),
                log=MW.encode_log(w), slots=np.stack([MW.encode_mps(w, kf.mvpMapPoints) for kf in w.kfs]),
                bad=np.array([p.mbBad for p in w.mps], bool), desc=np.stack([p.mDescriptor for p in w.mps]))


def assert_state(got, want, tag=""):
    for k in STATE:
        assert np.array_equal(got[k], want[k]), (tag, k)


def golden_state(g, n, prefix="n"):
    return {k: g[f"{prefix}{n}_{k}"] for k in STATE}


def drive_ckf(w, g, search):
    """compute_sim3's search on keyframe 1 with every map point of the world and the golden's pre-filled vpMatched:
    search(kf, Scw, points, vpMatched, th) returns (nmatches, vpMatched); gives (nmatches, encoded vpMatched)."""
    import matcher_world as MW
    vm = [None if i < 0 else w.mps[int(i)] for i in g["ckf_pre"]]
    n, vm = search(w.kfs[1], g["ckf_Scw"], list(w.mps), vm, TH_CKF)
    return int(n), MW.encode_mps(w, vm)
