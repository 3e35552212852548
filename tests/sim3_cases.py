"""Cases for k_sim3_search on the geometry of tests/fuse_cases.py (fx = fy = 64, 16 px cells, four levels with the scale
factors 1, 1.25, 1.5, 2; th = 3).  A search is a target keyframe, a two-stage pose and a list of rows of one shared
point table; poses are made of quarter turns, powers of two and dyadic translations, so a point made by `spt(u, v,
pose)` lands on exactly (u, v) and every gate is decided by small dyadic numbers.  Each case carries its claim as a
`check` over the array oracle's flat results, which tests/test_sim3_cpu.py runs, so the GPU test that compares the
kernel with the oracle cannot pass on inputs that miss the situation.

A case: name, frames (fuse_oracle keyframe dicts), pt_f64 / pt_desc (the point table), srch_f64 / srch_kf / items
(per search its 28 scalars, its target and its rows of the table), th, eps, check(best_idx, best_dist, status) and
marked (the items built to come back ORBFE_FUSE_MARGINAL; no other item may).

Also the drivers of the golden tests/golden/sim3_many.npz, shared by its generator and the tests.
"""
from __future__ import annotations

import math

import numpy as np

import fuse_cases as FC
import fuse_oracle as O
import sim3_oracle as S3
from bow_match_cases import D, R
from fuse_cases import EYE, FX, FY, TH, KfBuilder

CHUNK, GROUP = FC.CHUNK, FC.GROUP
TURN_Z = [0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]   # a quarter turn about z
TURN_Y = [0.0, 0.0, 1.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0]   # a quarter turn about y
ZERO = (0.0, 0.0, 0.0)


def mk_pose(Rw=EYE, tw=ZERO, s=1.0, Rs=EYE, t=ZERO, K=(FX, FY, 0.0, 0.0)):
    """c1 = Rw p + tw, c = (s Rs) c1 + t, projected with K; Rw and Rs orthogonal, s a power of two."""
    return dict(Rw=list(Rw), tw=list(tw), s=float(s), Rs=list(Rs), t=list(t), K=list(K))


IDENT = mk_pose()


def row(P):
    return P["K"] + P["Rw"] + P["tw"] + [P["s"] * x for x in P["Rs"]] + P["t"]


def _m(v):
    return np.array(v, np.float64).reshape(3, 3)


def spt(u, v, P=IDENT, z=1.0, level=0, desc=None, min_f=0.5, max_f=2.0, cos=1.0, q=None):
    """A point that search pose P projects to exactly (u, v) from depth z: its row of nine doubles and its
    descriptor.  min_f / max_f: the invariance distances as multiples of |c|; cos: the cosine between the normal
    and the point's direction from the world origin (not read by the kernel); q: the level quotient (default
    level - 0.5)."""
    fx, fy, cx, cy = P["K"]
    c = np.array([(u - cx) * z / fx, (v - cy) * z / fy, z])
    dist = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    c1 = _m(P["Rs"]).T @ (c - np.array(P["t"])) / P["s"]
    p = _m(P["Rw"]).T @ (c1 - np.array(P["tw"]))
    back = _m(row(P)[16:25]) @ (_m(P["Rw"]) @ p + np.array(P["tw"])) + np.array(P["t"])
    assert (back == c).all(), "the pose does not invert exactly"
    n = float(np.linalg.norm(p))
    nrm = [float(x) * cos / n for x in p] if n > 0 else [0.0, 0.0, 1.0]
    q = level - 0.5 if q is None else q
    return [float(x) for x in p] + nrm + [min_f * dist, max_f * dist, dist * 1.25 ** q], (D() if desc is None else desc)


def _case(name, frames, points, srch, srch_kf, items, check, th=TH, eps=O.EPS_F64, marked=()):
    return dict(name=name, frames=[f.build() if isinstance(f, KfBuilder) else f for f in frames],
                pt_f64=np.array([p[0] for p in points], np.float64).reshape(-1, O.PT_F64),
                pt_desc=np.array([p[1] for p in points], np.uint8).reshape(-1, 32),
                srch_f64=[row(P) if isinstance(P, dict) else list(P) for P in srch], srch_kf=list(srch_kf),
                items=[list(it) for it in items], th=th, eps=eps, check=check, marked=list(marked))


def arrays(case):
    return S3.join(case["frames"], case["pt_f64"], case["pt_desc"], case["srch_f64"], case["srch_kf"], case["items"],
                   case["th"], case["eps"])


def oracle(case, **kw):
    return S3.search(arrays(case), **kw)


def geom(case, i, **kw):
    """The oracle's phase 1 of item i: (status, window or None)."""
    a = arrays(case)
    return S3._window(a, S3.search_of(a, i), i, **kw)[2]


def _expect(bi, bd, want):
    """want: {item: (idx, dist)}; every other item has no candidate."""
    assert bi.ndim == 1 and bi.shape == bd.shape
    for i in range(len(bi)):
        assert (int(bi[i]), int(bd[i])) == want.get(i, (-1, -1)), (i, bi[i], bd[i])


def _one_feature():
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9))
    return kf


# ---- the pose ------------------------------------------------------------------------------------------------------

POSE2 = mk_pose(Rw=TURN_Z, tw=(0.5, -0.25, 2.0), s=1.0, Rs=TURN_Y, t=(0.25, 0.5, 3.0))


def two_stage_pose(eps=O.EPS_F64, name="two_stage_pose"):
    """Quarter turns about two axes and two translations: the point lands on the feature only through both stages in
    order; either stage alone sends it elsewhere."""
    c = _case(name, [_one_feature()], [spt(100.5, 100.25, POSE2)], [POSE2], [0], [[0]], None, eps=eps)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {0: (0, 1)})
        assert geom(c, 0)[1][:2] == (100.5, 100.25)
        assert not st.any()
    c["check"] = check
    return c


def scale_changes_the_level():
    """s = 2 doubles |c| against the world distance.  mfMaxDistance puts the camera distance's quotient at -2.6
    (level 0, which takes octave 0 only) and the world distance's at 0.5 (level 1, which also takes the closer
    feature of octave 1)."""
    P = mk_pose(s=2.0)
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1), octave=1)
    kf.add(101.0, 100.0, D(1, 2, 3), octave=0)
    c = _case("scale_changes_the_level", [kf], [spt(100.5, 100.25, P, q=0.5 - math.log(2.0) / math.log(1.25),
                                                    min_f=0.25)], [P], [0], [[0]], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {0: (1, 3)})
        assert geom(c, 0)[1][5] == 0 and geom(c, 0, world_distance=True)[1][5] == 1
        assert not st.any()
    c["check"] = check
    return c


def normal_away():
    c = _case("normal_pointing_away_still_matches", [_one_feature()], [spt(100.5, 100.25, cos=-1.0)], [IDENT], [0],
              [[0]], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {0: (0, 1)})
        assert c["pt_f64"][0][5] < 0 and not st.any()
    c["check"] = check
    return c


def _clean():
    """Two keyframes and two searches with results in both, the clean twin of the two not-read cases."""
    a, b = KfBuilder(), KfBuilder()
    a.add(100.0, 100.0, D(9))
    b.add(300.0, 200.0, D(9, 10))
    pts = [spt(100.5, 100.25, POSE2), spt(300.5, 200.25)]
    return _case("clean", [a, b], pts, [POSE2, IDENT], [0, 1], [[0, 1], [1, 0]], None)


def slots_not_read():
    junk = [float("nan"), float("inf"), -float("inf")]
    clean = _clean()
    want = oracle(clean)
    assert (want[0] >= 0).sum() == 2 and not want[2].any()

    def check(bi, bd, st):
        for got, w in zip((bi, bd, st), want):
            assert np.array_equal(got, w)
    n = dict(clean, name="normal_slots_are_not_read", check=check)
    n["pt_f64"] = clean["pt_f64"].copy()
    n["pt_f64"][:, 3:6] = [junk, junk[::-1]]
    k = dict(clean, name="keyframe_pose_and_intrinsics_slots_are_not_read", check=check)
    k["frames"] = [dict(f, f64=np.array((junk * 7)[:20] + list(f["f64"][20:]), np.float64)) for f in clean["frames"]]
    return [n, k]


def intrinsics_from_the_search():
    """The target's own block says fx = fy = 32, cx = cy = 8, under which the point would land on (58.25, 58.125),
    where the closer descriptor sits."""
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1, 2, 3))
    kf.add(58.0, 58.0, D(1))
    f = kf.build()
    f["f64"][0:4] = [32.0, 32.0, 8.0, 8.0]
    c = _case("intrinsics_from_the_search", [f], [spt(100.5, 100.25)], [IDENT], [0], [[0]], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {0: (0, 3)})
        assert geom(c, 0, target_intrinsics=True)[1][:2] == (58.25, 58.125)
        assert not st.any()
    c["check"] = check
    return c


# ---- the depth gate ---------------------------------------------------------------------------------------------------

def depth_cases():
    """Stage 2 gives z == 0 (the third row of sR and of t is zero, so every term is and the bound with them) with
    x != 0 (u inf) and with x == 0 (u NaN); and z = -2^-20 and +2^-20 at the same pixel through t = (0, 0, -1)."""
    flat = dict(IDENT, Rs=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
    P = mk_pose(t=(0.0, 0.0, -1.0))
    z = 2.0 ** -20
    front = spt(100.5, 100.25, P, z=z)
    behind = spt(100.5, 100.25, P, z=z)
    behind[0][0:3] = [-front[0][0], -front[0][1], 1.0 - z]
    ref = spt(100.5, 100.25)[0]
    pts = [(ref[:2] + [1.0] + ref[3:], D()), ([0.0, 0.0, 1.0] + ref[3:], D()), behind, front]
    c = _case("depth_zero_and_either_side", [_one_feature()], pts, [flat, P], [0, 0], [[0, 1], [2, 3]], None)

    def check(bi, bd, st, c=c, z=z):
        _expect(bi, bd, {3: (0, 1)})
        a = arrays(c)
        zs = [S3._stage(a["srch_f64"][s][16:25], a["srch_f64"][s][25:28], S3._stage(
            a["srch_f64"][s][4:13], a["srch_f64"][s][13:16], a["pt_f64"][i][:3], 0.0)[0], 0.0)[0][2]
              for s, i in ((0, 0), (0, 1), (1, 2), (1, 3))]
        assert zs == [0.0, 0.0, -z, z]
        assert not st.any()
    c["check"] = check
    return [c]


def distance_cases():
    """|c| exactly on the minimum (it passes, as the reference's min <= dist) and on the maximum: marked, since c is a
    rounded quantity.  A thousandth inside: not marked.  A thousandth outside: gated."""
    out = []
    for name, kw_at, kw_in, kw_out in (("dist_at_min", dict(min_f=1.0), dict(min_f=0.999), dict(min_f=1.001)),
                                       ("dist_at_max", dict(max_f=1.0), dict(max_f=1.001), dict(max_f=0.999))):
        pts = [spt(100.5, 100.25, POSE2, **kw) for kw in (kw_at, kw_in, kw_out)]
        c = _case(name, [_one_feature()], pts, [POSE2], [0], [[0, 1, 2]], None, marked=[0])

        def check(bi, bd, st, c=c, name=name):
            _expect(bi, bd, {0: (0, 1), 1: (0, 1)})
            dist = math.sqrt((1.5703125 ** 2 + 1.56640625 ** 2) + 1.0)
            assert c["pt_f64"][0][6 if name == "dist_at_min" else 7] == dist
            assert st.tolist() == [O.MARGINAL, 0, 0]
        c["check"] = check
        out.append(c)
    return out


def marginal_case():
    """A feature exactly one radius (3 px) from the second point's projection: |dx| == r is no candidate, and within
    rounding of being one."""
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1), cell=(6, 6))
    kf.add(303.5, 100.0, D(1), cell=(18, 6))
    kf.add(300.0, 100.0, D(1, 2), cell=(18, 6))
    kf.add(500.0, 100.0, D(1), cell=(31, 6))
    pts = [spt(100.5, 100.0, POSE2), spt(300.5, 100.0, POSE2), spt(500.25, 100.0, POSE2)]

    def check(bi, bd, st):
        _expect(bi, bd, {0: (0, 1), 1: (2, 2), 2: (3, 1)})
        assert st.tolist() == [0, O.MARGINAL, 0]
    return _case("marginal", [kf], pts, [POSE2], [0], [[0, 1, 2]], check, marked=[1])


# ---- the launch shape -------------------------------------------------------------------------------------------------

def _table():
    """A lattice keyframe of 20 features and a table of 80 points: row j looks at feature j % 20 from 3 + j // 20
    bits away."""
    kf = FC._lattice_kf(20)
    pts = [spt(50.5 + 40.0 * (j % 20 % 12), 60.25 + 40.0 * (j % 20 // 12), desc=D(*R(200, 200 + j // 20)))
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
    return _case(name, [kf], pts, [IDENT] * len(sizes), [0] * len(sizes), items, check)


def shared_points():
    """Two searches index the same rows in different orders, one with a repeat."""
    kf, pts = _table()
    items = [[0, 5, 41, 5, 19], [19, 41, 5, 0]]
    want = {i: (r % 20, 3 + r // 20) for i, r in enumerate(items[0] + items[1])}

    def check(bi, bd, st):
        _expect(bi, bd, want)
        assert bi[1] == bi[3] == bi[7] and items[0].count(5) == 2
    return _case("shared_points", [kf], pts[:42], [IDENT, IDENT], [0, 0], items, check)


def targets_case():
    """Two searches into keyframe 0 whose poses differ by a quarter of a unit along x (16 px), a keyframe no search
    targets, and a search into a keyframe without features."""
    def kf():
        k = KfBuilder()
        k.add(100.0, 100.0, D(1))
        k.add(116.0, 100.0, D(1, 2))
        return k
    shifted = mk_pose(t=(0.25, 0.0, 0.0))
    c = _case("two_poses_one_target_and_idle_and_empty_keyframes", [kf(), kf(), KfBuilder()], [spt(100.5, 100.25)],
              [IDENT, shifted, IDENT], [0, 0, 2], [[0], [0], [0]], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {0: (0, 1), 1: (1, 2)})
        assert geom(c, 1)[1][0] == 116.5 and 1 not in c["srch_kf"] and len(c["frames"][2]["xy"]) == 0
    c["check"] = check
    return c


def from_fuse(c0):
    """A case of k_fuse_search that does not hinge on the chi-square, the right coordinate or the viewing gate, as
    one identity search over all its points into its first keyframe."""
    P = len(c0["pt_f64"])
    c = dict(name="fuse_" + c0["name"], frames=c0["frames"][:1], pt_f64=c0["pt_f64"], pt_desc=c0["pt_desc"],
             srch_f64=[row(IDENT)], srch_kf=[0], items=[list(range(P))], th=c0["th"], eps=c0["eps"], marked=[])

    def check(bi, bd, st, c0=c0):
        c0["check"](bi.reshape(1, -1), bd.reshape(1, -1), st.reshape(1, -1))
        assert not st.any()
    c["check"] = check
    return c


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        taken = (FC.tie_cases() + [FC.window_case(L) for L in (15, 16, 17, 65)] + FC.clamp_cases()
                 + FC.early_return_cases() + FC.level_cases() + FC.octave_cases() + [FC.no_cell(), FC.radius_case()])
        _ALL = ([two_stage_pose(), scale_changes_the_level(), normal_away()] + slots_not_read()
                + [intrinsics_from_the_search()] + depth_cases() + distance_cases() + [marginal_case()]
                + [ragged_case((1, 0, 255, 256, 0, 257, 0), "ragged_0_1_255_256_257"), ragged_case((0, 0), "zero_items"),
                   ragged_case((), "zero_searches"), shared_points(), targets_case()]
                + [from_fuse(c) for c in taken] + [two_stage_pose(O.EPS_F32, "eps_of_float32")])
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


# ---- search_by_sim3 on a matcher_world world (shared by the golden's generator and the tests) -----------------------

N_PAIRS = (1, 3, 6)
SCALES = (1.0, 1.1, 0.9)
TH_SIM3 = 7.5


def sim3_of(w, j, s12, rng=None, dtype=np.float64):
    """(R12, t12) between keyframes 0 and j as matcher_world.drive builds them, t12 moved by a seeded perturbation."""
    k1, k2 = w.kfs[0], w.kfs[j]
    R1, t1 = k1.get_rotation().astype(np.float64), k1.get_translation().astype(np.float64)
    R2, t2 = k2.get_rotation().astype(np.float64), k2.get_translation().astype(np.float64)
    R12 = R1 @ R2.T
    t12 = s12 * (t1 - R12 @ t2)
    if rng is not None:
        t12 = t12 + rng.normal(0, 0.01, (3, 1))
    return R12.astype(dtype), t12.astype(dtype)


def prefill(w, j, rng, share=0.25):
    """Encoded vpMatches12 before the call: about `share` of keyframe 0's slots hold a map point, half of them one
    that keyframe j observes (so its index there is valid), the others any point."""
    k1, k2 = w.kfs[0], w.kfs[j]
    seen = [p for p in k2.mvpMapPoints if p is not None]
    pre = np.full(k1.N, -1, np.int32)
    for i in rng.choice(k1.N, int(share * k1.N), replace=False).tolist():
        p = seen[int(rng.integers(len(seen)))] if rng.random() < 0.5 else w.mps[int(rng.integers(len(w.mps)))]
        pre[i] = w.mp_id(p)
    return pre


def make_sim3s(w, seed, dtype=np.float64):
    """The golden's per-pair arrays for keyframes 1.. of the world: sim3_s{j}, sim3_R{j}, sim3_t{j}, sim3_pre{j}."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = {}
    for j in range(1, len(w.kfs)):
        s12 = SCALES[(j - 1) % 3]
        g[f"sim3_s{j}"] = np.float64(s12)
        g[f"sim3_R{j}"], g[f"sim3_t{j}"] = sim3_of(w, j, s12, rng, dtype)
        g[f"sim3_pre{j}"] = prefill(w, j, rng)
    return g


def pairs_of(w, g, n):
    """[(kf2, vpMatches12, s12, R12, t12)] for keyframes 1..n of a fresh world."""
    return [(w.kfs[j], [None if i < 0 else w.mps[int(i)] for i in g[f"sim3_pre{j}"]], float(g[f"sim3_s{j}"]),
             g[f"sim3_R{j}"], g[f"sim3_t{j}"]) for j in range(1, n + 1)]


def encode(w, res):
    """(n per pair, encoded vpMatches12 per pair) of a list of search_by_sim3 results."""
    import matcher_world as MW
    return [int(r[0]) for r in res], [MW.encode_mps(w, r[1]) for r in res]


def loop_single(single):
    """search_by_sim3_many as the loop of single calls."""
    def many(kf1, kfs2, vms, ss, Rs, ts, th):
        return [single(kf1, kf, v, s, R_, t, th) for kf, v, s, R_, t in zip(kfs2, vms, ss, Rs, ts)]
    return many


def drive(w, g, many, n):
    """search_by_sim3 from keyframe 0 to keyframes 1..n through many(kf1, kfs2, vpMatches12s, s12s, R12s, t12s, th);
    gives the encoded results."""
    prs = pairs_of(w, g, n)
    res = many(w.kfs[0], *[[p[c] for p in prs] for c in range(5)], TH_SIM3)
    return encode(w, res)
