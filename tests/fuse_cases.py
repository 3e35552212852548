"""Cases for k_fuse_search: a geometry in which every gate is decided by small dyadic numbers, crafted descriptors
(bit flips of one base row give exact Hamming distances) and hand-written grids.  Each case carries the claim it
exists for as a `check` over the array oracle's results, which tests/test_fuse_cpu.py runs, so the GPU test that
compares the kernel with the oracle cannot pass on inputs that miss the situation.

Geometry.  The standard keyframe has the identity pose, fx = fy = 64, cx = cy = 0, bf = 32, the image [0, 640) x
[0, 480) and a grid of 40 x 30 cells of 16 px (both inverses are 1 / 16, exact).  A point made by `pt(u, v)` lies at
depth 1 and projects to exactly (u, v) with ur = u - 32.  Four levels with the scale factors 1, 1.25, 1.5, 2 and the
inverse sigma squares 1, 1 / 2, 1 / 4, 1 / 8; th = 3, so the radii are 3, 3.75, 4.5 and 6.  `pt(level=L)` sets
mfMaxDistance = dist * 1.25 ** (L - 0.5): the level quotient is L - 0.5 and its ceil is L.

A case: name, frames (fuse_oracle keyframe dicts), pt_f64 / pt_desc, th, eps, check(best_idx, best_dist, status) and
marginal (True for the one case built to be marked).
"""
from __future__ import annotations

import math

import numpy as np

import fuse_oracle as O
from bow_match_cases import D, R, _filler

CHUNK = 256  # points per k_fuse_search workgroup (ORBFE_FUSE_CHUNK)
GROUP = 16   # lanes that share one point's candidates (kFuGroup)
FX = FY = 64.0
BF = 32.0
CELL = 16
COLS, ROWS = 40, 30
SCALE = [1.0, 1.25, 1.5, 2.0]
INV_SIG2 = [1.0, 0.5, 0.25, 0.125]
LSF = math.log(1.25)
TH = 3.0
EYE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


class KfBuilder:
    """A keyframe given feature by feature; a feature goes into the cell of its position (floor), into the cell
    named, or into none; a cell's list keeps the order of the calls unless `order` rearranges it."""

    def __init__(self, cols=COLS, rows=ROWS, bounds=(0.0, 640.0, 0.0, 480.0), inv=(1.0 / CELL, 1.0 / CELL),
                 inv_sigma2=INV_SIG2, scale=SCALE, R=EYE, t=(0.0, 0.0, 0.0), Ow=(0.0, 0.0, 0.0)):
        self.cols, self.rows, self.bounds, self.inv = cols, rows, bounds, inv
        self.inv_sigma2, self.scale, self.R, self.t, self.Ow = inv_sigma2, scale, R, t, Ow
        self.xy, self.octave, self.ur, self.desc, self.cells = [], [], [], [], {}

    def add(self, x, y, desc, octave=0, ur=-1.0, cell="auto"):
        i = len(self.xy)
        self.xy.append((float(x), float(y)))
        self.octave.append(octave)
        self.ur.append(float(ur))
        self.desc.append(desc)
        if cell == "auto":
            cell = (int(x // CELL), int(y // CELL))
        if cell is not None:
            self.cells.setdefault(cell, []).append(i)
        return i

    def build(self):
        n = len(self.xy)
        sizes = [len(self.cells.get((ix, iy), ())) for ix in range(self.cols) for iy in range(self.rows)]
        idx = [g for ix in range(self.cols) for iy in range(self.rows) for g in self.cells.get((ix, iy), ())]
        assert all(0 <= ix < self.cols and 0 <= iy < self.rows for ix, iy in self.cells)
        f64 = [FX, FY, 0.0, 0.0, BF] + list(self.R) + list(self.t) + list(self.Ow) + list(self.bounds) + list(
            self.inv) + [LSF]
        return dict(f64=np.array(f64, np.float64), i32=np.array([self.cols, self.rows, len(self.scale)], np.int32),
                    xy=np.array(self.xy, np.float64).reshape(n, 2), octave=np.array(self.octave, np.int32),
                    u_right=np.array(self.ur, np.float64), desc=np.array(self.desc, np.uint8).reshape(n, 32),
                    cell_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                    cell_idx=np.array(idx, np.int32), scale=np.array(self.scale, np.float64),
                    inv_sigma2=np.array(self.inv_sigma2, np.float64))


def pt(u, v, level=0, z=1.0, desc=None, min_f=0.5, max_f=2.0, cos=1.0, q=None):
    """A point that projects to exactly (u, v) in the standard keyframe from depth z (a power of two): its row of
    nine doubles and its descriptor.  min_f / max_f: the invariance distances as multiples of its distance; cos:
    the viewing cosine; q: the level quotient (default level - 0.5)."""
    X, Y = u * z / FX, v * z / FY
    dist = math.sqrt((X * X + Y * Y) + z * z)
    n = [c * cos / dist for c in (X, Y, z)] if dist > 0 else [0.0, 0.0, 1.0]
    q = level - 0.5 if q is None else q
    return [X, Y, z] + n + [min_f * dist, max_f * dist, dist * 1.25 ** q], (D() if desc is None else desc)


def _case(name, frames, points, check, th=TH, eps=O.EPS_F64, marginal=False):
    return dict(name=name, frames=[f.build() if isinstance(f, KfBuilder) else f for f in frames],
                pt_f64=np.array([p[0] for p in points], np.float64).reshape(-1, O.PT_F64),
                pt_desc=np.array([p[1] for p in points], np.uint8).reshape(-1, 32), th=th, eps=eps, check=check,
                marginal=marginal)


def arrays(case):
    return O.join(case["frames"], case["pt_f64"], case["pt_desc"], case["th"], case["eps"])


def oracle(case, **kw):
    return O.search(arrays(case), **kw)


def geom(case, k, i):
    """The oracle's phase 1 of item (k, i): (status, window or None)."""
    f = case["frames"][k]
    return O.geometry(f["f64"], f["i32"], f["scale"], case["pt_f64"][i], case["th"], case["eps"])


def _expect(bi, bd, want):
    """want: {(k, i): (idx, dist)}; every other item has no candidate."""
    for k in range(bi.shape[0]):
        for i in range(bi.shape[1]):
            assert (int(bi[k, i]), int(bd[k, i])) == want.get((k, i), (-1, -1)), (k, i, bi[k, i], bd[k, i])


# ---- sizes ------------------------------------------------------------------------------------------------------

def one_one():
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1, 2, 3))
    return _case("one_point_one_feature", [kf], [pt(100.5, 100.25)], lambda bi, bd, st: _expect(bi, bd, {(0, 0): (0, 3)}))


def zero_points():
    kf = KfBuilder()
    kf.add(100.0, 100.0, D())
    return _case("zero_points", [kf], [], lambda bi, bd, st: _assert(bi.shape == (1, 0)))


def zero_features():
    return _case("keyframe_without_features", [KfBuilder()], [pt(100.5, 100.25), pt(300.5, 200.25)],
                 lambda bi, bd, st: _expect(bi, bd, {}))


def no_keyframes():
    return _case("no_keyframes", [], [pt(100.5, 100.25)], lambda bi, bd, st: _assert(bi.shape == (0, 1)))


def _assert(cond):
    assert cond


def _lattice_kf(n, shift=0.0):
    """n features on a lattice 40 px apart; feature j has bits [8 j, 8 j + 3) flipped (n <= 32)."""
    kf = KfBuilder()
    for j in range(n):
        kf.add(50.0 + 40.0 * (j % 12) + shift, 60.0 + 40.0 * (j // 12), D(*R(8 * j, 8 * j + 3)))
    return kf


def chunk_case(P):
    """P points of one keyframe; point i looks at feature i % 20 and differs from it in 3 + (i % 4) bits."""
    kf = _lattice_kf(20)
    pts, want = [], {}
    for i in range(P):
        j = i % 20
        pts.append(pt(50.5 + 40.0 * (j % 12), 60.25 + 40.0 * (j // 12), desc=D(*R(200, 200 + i % 4))))
        want[(0, i)] = (j, 3 + i % 4)
    return _case(f"points_{P}", [kf], pts, lambda bi, bd, st: _expect(bi, bd, want))


def ragged_case(K):
    """K keyframes of 1 + 3 k features (feature positions shifted by k / 4 px) share 7 points."""
    kfs = [_lattice_kf(1 + 3 * k, shift=0.25 * (k % 5)) for k in range(K)]
    pts = [pt(50.5 + 40.0 * j, 60.25, desc=D(255)) for j in range(7)]
    want = {(k, j): (j, 4) for k in range(K) for j in range(7) if j < min(1 + 3 * k, 12)}
    return _case(f"ragged_{K}", kfs, pts, lambda bi, bd, st: _expect(bi, bd, want))


# ---- the window ---------------------------------------------------------------------------------------------------

def clamp_cases():
    out = []
    for name, (u, v), (fx_, fy_), edge in (("col_0", (1.5, 100.25), (2.0, 100.0), (0, None)),
                                           ("col_last", (638.5, 100.25), (637.0, 100.0), (1, COLS - 1)),
                                           ("row_0", (100.5, 1.25), (100.0, 2.0), (2, None)),
                                           ("row_last", (100.5, 478.25), (100.0, 477.0), (3, ROWS - 1))):
        kf = KfBuilder()
        kf.add(fx_, fy_, D(9))
        c = _case(f"clamp_{name}", [kf], [pt(u, v)], None)

        def check(bi, bd, st, c=c, edge=edge, u=u, v=v):
            _expect(bi, bd, {(0, 0): (0, 1)})
            w = geom(c, 0, 0)[1]
            raw = [math.floor((u - TH) / CELL), math.ceil((u + TH) / CELL), math.floor((v - TH) / CELL),
                   math.ceil((v + TH) / CELL)]
            lim = (0, COLS - 1, 0, ROWS - 1)
            assert w[8 + edge[0]] == lim[edge[0]] != raw[edge[0]]  # the clamp acted
        c["check"] = check
        out.append(c)
    return out


def early_return_cases():
    """In the image but outside a grid that covers only its first 160 x 160 px (10 x 10 cells), and radii below
    zero (th = -20), which put the window's upper end below cell 0."""
    out = []
    for name, (u, v), th in (("x0", (300.5, 100.25), TH), ("x1", (1.5, 100.25), -20.0), ("y0", (100.5, 300.25), TH),
                             ("y1", (100.5, 1.25), -20.0)):
        kf = KfBuilder(cols=10, rows=10)
        kf.add(100.0, 100.0, D(9))
        kf.add(2.0, 100.0, D(9))
        kf.add(100.0, 2.0, D(9))
        c = _case(f"early_return_{name}", [kf], [pt(u, v)], None, th=th)

        def check(bi, bd, st, c=c, name=name, u=u, v=v, th=th):
            _expect(bi, bd, {})
            assert geom(c, 0, 0)[1] is None
            r = th * 1.0
            raw = dict(x0=math.floor((u - r) / CELL) >= 10, x1=math.ceil((u + r) / CELL) < 0,
                       y0=math.floor((v - r) / CELL) >= 10, y1=math.ceil((v + r) / CELL) < 0)
            assert [k for k, hit in raw.items() if hit] == [name]
        c["check"] = check
        out.append(c)
    return out


def image_bound_cases():
    """u == mnMinX is inside, u == mnMaxX outside.  Both at u = 0, where every summed term of the projection is zero
    and so is the bound: an exact equality anywhere else is within rounding of the bound and marginal by design."""
    kf = KfBuilder()
    kf.add(1.0, 100.0, D(9))
    inside = _case("u_equals_min_x", [kf], [pt(0.0, 100.25)], lambda bi, bd, st: _expect(bi, bd, {(0, 0): (0, 1)}))
    kf2 = KfBuilder(bounds=(-640.0, 0.0, 0.0, 480.0))
    kf2.add(-1.0, 100.0, D(9), cell=(39, 6))
    c = _case("u_equals_max_x", [kf2], [pt(0.0, 100.25), pt(-0.5, 100.25)], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {(0, 1): (0, 1)})  # half a pixel further left the same feature is found
        assert geom(c, 0, 0)[1] is None and c["pt_f64"][0][0] == 0.0
    c["check"] = check
    return [inside, c]


def depth_cases():
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9))
    behind = pt(100.5, 100.25)
    behind[0][0:3] = [-behind[0][0], -behind[0][1], -1.0]  # projects to the same pixel from behind the camera
    flat0 = (pt(100.5, 100.25)[0][:2] + [0.0] + pt(100.5, 100.25)[0][3:], D())   # z == 0, x != 0: u is inf
    flat1 = ([0.0, 0.0, 0.0] + pt(100.5, 100.25)[0][3:], D())                     # z == 0, x == 0: u is NaN
    c = _case("depth_negative_and_zero", [kf], [behind, flat0, flat1, pt(100.5, 100.25)], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {(0, 3): (0, 1)})
        assert c["pt_f64"][0][2] < 0 and c["pt_f64"][1][2] == 0.0 == c["pt_f64"][2][2]
    c["check"] = check
    return [c]


def distance_cases():
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9))
    pts = [pt(100.5, 100.25, min_f=1.001), pt(100.5, 100.25, min_f=0.999), pt(100.5, 100.25, max_f=0.999),
           pt(100.5, 100.25, max_f=1.001), pt(100.5, 100.25, cos=0.49), pt(100.5, 100.25, cos=0.51)]
    return [_case("distances_and_viewing_either_side", [kf], pts,
                  lambda bi, bd, st: _expect(bi, bd, {(0, 1): (0, 1), (0, 3): (0, 1), (0, 5): (0, 1)}))]


def level_cases():
    """Quotients -2.5 and 7.5 clamp to levels 0 and 3; the features' octaves tell which level was used."""
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(9), octave=0)
    kf.add(101.0, 100.0, D(9, 10), octave=3)
    c = _case("level_clamped_low_and_high", [kf], [pt(100.5, 100.25, q=-2.5), pt(100.5, 100.25, q=7.5)], None)

    def check(bi, bd, st, c=c):
        _expect(bi, bd, {(0, 0): (0, 1), (0, 1): (1, 2)})
        assert geom(c, 0, 0)[1][7] == 0 and geom(c, 0, 1)[1][7] == 3
    c["check"] = check
    return [c]


def octave_cases():
    """Level 2 takes octaves 1 and 2; the closest descriptors sit at octaves 0 and 3."""
    kf = KfBuilder()
    kf.add(101.0, 100.0, D(1), octave=0)
    kf.add(101.0, 101.0, D(1, 2, 3, 4, 5), octave=1)
    kf.add(102.0, 100.0, D(200, 201, 202, 203, 204, 205), octave=2)
    kf.add(102.0, 101.0, D(1, 2), octave=3)
    pts = [pt(101.5, 100.25, level=2), pt(101.5, 100.25, level=2, desc=D(*R(200, 206)))]
    return [_case("octave_window", [kf], pts, lambda bi, bd, st: _expect(bi, bd, {(0, 0): (1, 5), (0, 1): (2, 0)}))]


def chi_cases():
    """Level 0, inverse sigma square 1: the chi-square is the squared error itself.  Mono: 2^2 + 1^2 = 5 passes,
    2^2 + 1.5^2 = 6.25 fails.  Stereo (ur = u - 32): 4 + 1 + 1.5^2 = 7.25 passes, 4 + 1 + 2^2 = 9 fails.  In every
    pair the failing feature has the closer descriptor."""
    out = []
    u, v = 100.5, 100.25
    for name, good, bad in (("mono", (2.0, 1.0, None), (2.0, 1.5, None)), ("stereo", (2.0, 1.0, 1.5), (2.0, 1.0, 2.0))):
        kf = KfBuilder()
        for (ex, ey, er), desc in ((bad, D(1)), (good, D(1, 2, 3))):
            kf.add(u - ex, v - ey, desc, ur=-1.0 if er is None else (u - BF) - er, cell=(6, 6))
        out.append(_case(f"chi_square_{name}", [kf], [pt(u, v)], lambda bi, bd, st: _expect(bi, bd, {(0, 0): (1, 3)})))
    return out


def u_right_zero():
    """A right coordinate of 0.0 is stereo: with u = 33.5 its third term is 1.5^2 and 2.2^2 + 1 + 2.25 = 8.09 fails
    7.8, while the same offsets as a mono feature (4.84 + 1 = 5.84) pass 5.99."""
    u, v = 33.5, 100.25
    kf = KfBuilder()
    kf.add(u - 2.2, v - 1.0, D(1), ur=0.0, cell=(1, 6))
    kf.add(u + 2.2, v + 1.0, D(1, 2, 3), ur=-1.0, cell=(1, 6))
    return _case("u_right_zero_is_stereo", [kf], [pt(u, v)], lambda bi, bd, st: _expect(bi, bd, {(0, 0): (1, 3)}))


def no_cell():
    kf = KfBuilder()
    kf.add(100.0, 100.0, D(1), cell=None)
    kf.add(101.0, 100.0, D(1, 2, 3))
    return _case("feature_in_no_cell", [kf], [pt(100.5, 100.25)], lambda bi, bd, st: _expect(bi, bd, {(0, 0): (1, 3)}))


def radius_case():
    """Level 3, radius 6: the closer descriptor is 6.5 px away in the same cell; its chi-square alone would pass."""
    kf = KfBuilder()
    kf.add(107.0, 100.25, D(1), octave=3, cell=(6, 6))
    kf.add(101.5, 100.25, D(1, 2, 3), octave=3, cell=(6, 6))
    return _case("radius_gate", [kf], [pt(100.5, 100.25, level=3)], lambda bi, bd, st: _expect(bi, bd, {(0, 0): (1, 3)}))


# ---- ties: the earliest visited wins --------------------------------------------------------------------------

def tie_cases():
    kf = KfBuilder()
    kf.add(112.5, 100.0, D(1, 2))   # index 0 in column 7: visited after column 6
    kf.add(111.5, 100.0, D(3, 4))   # index 1 in column 6
    two = _case("tie_in_two_cells", [kf], [pt(112.0, 100.25)], lambda bi, bd, st: _expect(bi, bd, {(0, 0): (1, 2)}))
    kf = KfBuilder()
    for j, d in enumerate((D(1, 2), D(1, 2, 3), D(3, 4))):
        kf.add(100.0 + j, 100.0, d, cell=None)
    kf.cells[(6, 6)] = [2, 1, 0]    # stored order: 2 first, though 0 has the same distance
    one = _case("tie_in_one_unsorted_cell", [kf], [pt(100.5, 100.25)], lambda bi, bd, st: _expect(bi, bd, {(0, 0): (2, 2)}))
    return [two, one]


def window_case(L):
    """L candidates pass every gate in a level-3 window (radius 6) spread over the cells of one column; the best
    descriptor is the last visited, the second best the first, and two equal third-best sit in between."""
    kf = KfBuilder()
    u, v = 112.5, 112.25
    offs = [(0.25 * a, 0.25 * b) for a in range(-8, 9) for b in range(-8, 9)][:L]
    offs.sort(key=lambda o: (int((u + o[0]) // CELL), int((v + o[1]) // CELL)))  # visiting order of their cells
    for j, (dx, dy) in enumerate(offs):
        d = D(1, 2) if j == L - 1 else D(1, 2, 3) if j == 0 else D(*R(100, 104)) if j in (L // 3, L // 2) else _filler(j)
        kf.add(u + dx, v + dy, d, octave=3 if j % 2 else 2)
    order = [g for ix in range(COLS) for iy in range(ROWS) for g in kf.cells.get((ix, iy), ())]
    assert order == list(range(L))
    c = _case(f"window_{L}", [kf], [pt(u, v, level=3), pt(u, v, level=3, desc=D(*R(100, 104), 1, 2, 3, 4, 5, 6, 7, 8, 9))], None)

    def check(bi, bd, st, L=L):
        want = {(0, 0): (L - 1, 2)}
        if L > 3:
            want[(0, 1)] = (L // 3, 9)   # the earlier of the two equal ones
        else:
            want[(0, 1)] = (int(bi[0, 1]), int(bd[0, 1]))
        _expect(bi, bd, want)
    c["check"] = check
    return c


# ---- the marginal bit ----------------------------------------------------------------------------------------------

def marginal_case():
    """inv_sigma2[0] = 5.99 and an error of exactly one pixel: the chi-square equals its threshold."""
    kf = KfBuilder(inv_sigma2=[5.99, 0.5, 0.25, 0.125])
    kf.add(100.0, 100.0, D(1), cell=(6, 6))
    kf.add(300.0, 100.5, D(1), cell=(18, 6))
    kf.add(500.0, 100.0, D(1), cell=(31, 6))
    pts = [pt(100.5, 100.0), pt(300.0, 101.5), pt(500.25, 100.0)]   # chi: 0.25 * 5.99, 5.99, 0.0625 * 5.99

    def check(bi, bd, st):
        _expect(bi, bd, {(0, 0): (0, 1), (0, 1): (1, 1), (0, 2): (2, 1)})
        assert st.tolist() == [[0, O.MARGINAL, 0]]
    return _case("marginal", [kf], pts, check, marginal=True)


def eps_f32_case():
    """The float32 unit of rounding on the standard geometry: no decision comes within the wider bound."""
    c = one_one()
    c.update(name="eps_of_float32", eps=O.EPS_F32)
    return c


# ---- keyframes with real poses, in both dtypes ---------------------------------------------------------------------

class Z:
    """A dict with the .files of an npz, which matcher_world.build reads."""

    def __init__(self, d):
        self._d, self.files = d, list(d.keys())

    def __getitem__(self, k):
        return self._d[k]


def pose_world(dtype, seed=5, n=60, n_mp=40):
    """(keyframes, points) of a small matcher_world world whose poses and positions are of `dtype`."""
    import matcher_world as MW
    z = MW.make_world(np.random.Generator(np.random.PCG64(seed)), n_kf=3, n=n, n_mp=n_mp)
    w = MW.build(Z(z))
    for kf in w.kfs:
        kf.Tcw = kf.Tcw.astype(dtype)
    for p in w.mps:
        p._pos, p._normal = p._pos.astype(dtype), p._normal.astype(dtype)
    return w


def pose_case(dtype):
    w = pose_world(dtype)
    pts = [p for p in w.mps if not p.is_bad()]
    a = O.pack(w.kfs[1:], pts, TH)
    c = dict(name=f"poses_{np.dtype(dtype).name}", frames=[O.pack_kf(kf) for kf in w.kfs[1:]], pt_f64=a["pt_f64"],
             pt_desc=a["pt_desc"], th=TH, eps=a["eps"], marginal=False, world=w, points=pts)

    def check(bi, bd, st, c=c, dtype=dtype):
        assert c["eps"] == (O.EPS_F32 if dtype == np.float32 else O.EPS_F64)
        found = 0
        for k, kf in enumerate(c["world"].kfs[1:]):
            for i, p in enumerate(c["points"]):
                if st[k, i]:
                    continue
                dist, idx = O.single_item(kf, p, TH)
                assert (idx, dist if idx >= 0 else -1) == (int(bi[k, i]), int(bd[k, i])), (k, i)
                found += idx >= 0
        assert found > 10
    c["check"] = check
    return c


# ---- LocalMapping.search_in_neighbors on a matcher_world world (shared by the golden's generator and the tests) ----

N_NEIGH = (1, 3, 6)
N_KF, N, N_MP = 7, 300, 220


def clone_world(seed, n_kf=N_KF, n=N, n_mp=N_MP):
    """Arrays of a matcher_world world of n_kf keyframes in which a share of the neighbours' slots holds a clone of
    the map point they re-observe (nearly the same position, a noisy descriptor): fusing then replaces points."""
    import matcher_world as MW
    N_KF, N_MP = n_kf, n_mp
    rng = np.random.Generator(np.random.PCG64(seed))
    z = MW.make_world(rng, n_kf=n_kf, n=n, n_mp=n_mp)
    pos, normal, desc = [z["mp_pos"]], [z["mp_normal"]], [z["mp_desc"]]
    clone = {}
    obs = z["obs"].tolist()
    at = {tuple(o): r for r, o in enumerate(obs)}
    for j in range(1, N_KF):
        slots = z[f"kfmp{j}"]
        for i in np.flatnonzero(slots >= 0).tolist():
            k = int(slots[i])
            if rng.random() < 0.55:
                continue
            if k not in clone:
                clone[k] = N_MP + len(clone)
                pos.append((z["mp_pos"][k] + rng.normal(0, 0.002, 3).astype(np.float32))[None])
                normal.append(z["mp_normal"][k][None])
                desc.append(MW.noisy_desc(rng, z["mp_desc"][k], int(rng.integers(0, 10)))[None])
            slots[i] = clone[k]
            obs[at[(k, j, i)]] = [clone[k], j, i]
    src = np.array(sorted(clone, key=clone.get), np.int64)
    z["mp_pos"], z["mp_normal"], z["mp_desc"] = np.concatenate(pos), np.concatenate(normal), np.concatenate(desc)
    for key in ("mp_min", "mp_max", "mp_bad"):
        z[key] = np.concatenate([z[key], z[key][src]])
    z["mp_bad"][N_MP:] = False
    z["obs"] = np.array(obs, np.int32).reshape(-1, 3)
    return z




def load_world(g):
    """A fresh world of a golden file's arrays (tests/golden/fuse_many.npz)."""
    import matcher_world as MW
    return MW.build(g)


def pooled_points(targets):
    """vpFuseCandidates of LocalMapping.py:362-373: the targets' map points, each once, bad ones left out."""
    cands, seen = [], set()
    for kf in targets:
        for p in kf.get_map_point_matches():
            if not p or p.is_bad() or id(p) in seen:
                continue
            seen.add(id(p))
            cands.append(p)
    return cands


def drive(w, fuse, n_neigh):
    """The two fusion calls of search_in_neighbors with keyframe 0 as the current one and keyframes 1..n_neigh as
    the targets; fuse(kfs, points, th) returns the list of fuse_pkf_mp's return values."""
    cur, targets = w.kfs[0], w.kfs[1:1 + n_neigh]
    r1 = fuse(targets, cur.get_map_point_matches(), TH)
    r2 = fuse([cur], pooled_points(targets), TH)
    return list(r1) + list(r2)


def world_state(w, returns):
    import matcher_world as MW
    return dict(ret=np.array(returns, np.int32), log=MW.encode_log(w),
                slots=np.stack([MW.encode_mps(w, kf.mvpMapPoints) for kf in w.kfs]),
                bad=np.array([p.mbBad for p in w.mps], bool), desc=np.stack([p.mDescriptor for p in w.mps]))


def assert_state(got, want, tag=""):
    for k in ("ret", "log", "slots", "bad", "desc"):
        assert np.array_equal(got[k], want[k]), (tag, k)


def golden_state(g, n):
    return {k: g[f"n{n}_{k}"] for k in ("ret", "log", "slots", "bad", "desc")}


def oracle_fuse(stats=None):
    """fuse(kfs, points, th) by the array oracle and its replay."""
    return lambda kfs, pts, th: O.replay(kfs, pts, th, stats=stats)


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = ([one_one(), zero_points(), zero_features(), no_keyframes()]
                + [chunk_case(P) for P in (CHUNK - 1, CHUNK, CHUNK + 1)] + [ragged_case(K) for K in (1, 2, 9)]
                + clamp_cases() + early_return_cases() + image_bound_cases() + depth_cases() + distance_cases()
                + level_cases() + octave_cases() + chi_cases() + [u_right_zero(), no_cell(), radius_case()]
                + tie_cases() + [window_case(L) for L in (1, 63, 64, 65, 129)] + [marginal_case(), eps_f32_case()]
                + [pose_case(np.float32), pose_case(np.float64)])
    return _ALL
