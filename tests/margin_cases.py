"""Flip-point ladders for the five projection searches (proj_search<kMode> in pyorbslam_amd/csrc/orbfe_fuse.hip):
inputs that sit on a gate's threshold to within one unit in the last place of one input scalar, and around it.

The promise under test: every value a decision of the kernel compares carries a bound on how far the reference's own
value can lie from it, an item within that bound of a threshold is marked ORBFE_FUSE_MARGINAL, and an unmarked item
decides as the reference does.  The placed cases of fuse_cases.py, scw_cases.py, sim3_cases.py, fkf_cases.py and
local_search_cases.py are dyadic, so both arithmetics are exact there and the size of a bound decides nothing.  Here
nothing is dyadic.

Per (mode, precision) there is one small world: two targets (keyframes or frames; the Sim3 search has two searches
into one keyframe each) with a few dozen features, and START start items that pass every gate with room to spare.  A
ladder takes one start item and one scalar of its map point (a coordinate of the position, or the z component of the
normal), moves the scalar by bisection over its own dtype's representable values until the REFERENCE BODY's decision
at one gate differs between two adjacent values, and emits the scalar at +-2^j units in the last place around that
flip, j = 0 .. J: rung -1 and rung +1 are the two adjacent values, rung -2^j lies 2^j - 1 values before the first and
rung +2^j as many behind the second.  Every rung is one map point; nothing else of the world changes.

The reference body's decisions are read off the body itself, not restated: it runs under sys.settrace, which gives the
`return` it left by, what predict_scale returned, and the locals of get_features_in_area (the clamped window, the
radius, the candidates) and of fp_one (the radius factor, the winner, the two distances) as they return.

Gates and the scalar that is moved (p0, p1, p2: the position; n2: the normal's z):
    depth      p2 until the camera z changes sign
    bounds     p0 / p1 until u / v leaves by minX, maxX, minY, maxY
    distance   p2 until the distance leaves by the minimum or the maximum
    viewing    n2 until dot < 0.5 dist (fuse, scw) or the cosine < limit (local)
    radius     n2 until the cosine passes 0.998 (local)
    level      p2 until the predicted level changes: 0 | 1, an inner pair, and top - 1 | top
    window     p0 / p1 until one of the four window ends moves by a cell
    candidate  p0 / p1 until the start item's own feature leaves the square of radius r
    chi-square p0 until that feature fails the chi-square (7.8 with a right coordinate, 5.99 without; fuse)
    stereo     p0 until that feature fails |ur - uR| <= r (local)
Every ladder of the Sim3 search goes through both stages with |s| = 0.35 or 2.8, so the group "two-stage pose" is
the union of that mode's ladders.
"""
from __future__ import annotations

import inspect
import math
import sys

import numpy as np

import fkf_cases as KC
import fkf_oracle as FK
import fuse_oracle as O
import local_search_cases as LC
import local_search_oracle as LO
import matcher_world as MW
import scw_oracle as SO
import sim3_oracle as S3

MODES = ("fuse", "scw", "sim3", "fkf", "local")
PRECISIONS = ("f32", "f64")
DTYPE = {"f32": np.float32, "f64": np.float64}
EPS = {"f32": O.EPS_F32, "f64": O.EPS_F64}
J = 12                # rungs at +-2^0 .. +-2^J.  J - 1 closes 90 % of every group's ladders too, but leaves ladders
                      # open for their own bound alone; at J every ladder is closed
N_LADDERS = 16        # per (mode, gate, precision)
START = 16            # start items per target
TH = {"fuse": 3.0, "scw": 4.0, "sim3": 7.5, "fkf": 4.0}
TH_LOCAL = {"f32": 1.0, "f64": 2.0}    # th == 1 multiplies nothing in the reference, th != 1 does
LIMIT = 0.5
SIM3_SCALES = (0.35, 2.8)
Q_GUARD = 2.0 ** -40  # a rung whose level quotient lies closer to an integer than this is not sent to a device

GATES = {"fuse": ("depth", "bounds", "distance", "viewing", "level", "window", "candidate", "chi-square"),
         "scw": ("depth", "bounds", "distance", "viewing", "level", "window", "candidate"),
         "sim3": ("depth", "bounds", "distance", "level", "window", "candidate"),
         "fkf": ("bounds", "distance", "level", "window", "candidate"),
         "local": ("depth", "bounds", "distance", "viewing", "radius", "level", "window", "candidate", "stereo")}

# (mode, gate) pairs of the table for which no ladder exists, and why
CANNOT_BE_BUILT = {
    ("fkf", "depth"): "search_by_projection_f_kf_f has no depth gate: its body never compares the camera z with "
                      "anything, so no decision of the reference flips where |zc| passes the kernel's bound; the "
                      "kernel's mark around zc == 0 is pinned by fkf_cases.behind_case",
    **{(m, "window: early returns"): "a window that starts at or behind `cols` / `rows`, or ends before 0, needs "
       "u - r >= maxX or u + r < minX, which the image bounds rule out for every r > 0: the reference body cannot "
       "reach the four early returns of get_features_in_area; the placed cases reach them with their own grids"
       for m in MODES},
    **{(m, "level: the clamp"): "above levels - 1 and below 0 the reference clamps, so its decision does not change "
       "where the quotient passes those integers; the ladders flip 0 | 1, an inner pair and top - 1 | top instead"
       for m in MODES},
}

# the rung 2^j at which the mark disappears, as the median over each group's ladders: {mode: {gate: (f32, f64)}}.
# It is the table of DESIGN.md ("the ladders") and is asserted, to half a rung: a bound that changes size by a
# factor of two, in the kernel and the oracles alike, moves every ladder of its groups by a whole rung
LADDER_TABLE = {
    "fuse": {"depth": (6, 10), "bounds": (6, 9), "distance": (5, 9), "viewing": (6, 10), "level": (5, 9),
             "window": (6, 10), "candidate": (6, 10), "chi-square": (6, 10)},
    "scw": {"depth": (6, 10), "bounds": (6, 9.5), "distance": (5, 8.5), "viewing": (6, 10), "level": (5, 9),
             "window": (6, 10), "candidate": (6, 10)},
    "sim3": {"depth": (7, 10), "bounds": (6.5, 10), "distance": (6, 10), "level": (6, 10), "window": (6.5, 10),
             "candidate": (7, 10.5), "two-stage pose": (7, 10)},
    "fkf": {"bounds": (6, 10), "distance": (4.5, 9), "level": (5, 9), "window": (6, 10), "candidate": (6, 10)},
    "local": {"depth": (6, 10), "bounds": (6, 9), "distance": (5, 9), "viewing": (6, 9), "radius": (6, 9.5),
             "level": (5, 9), "window": (6, 10), "candidate": (6, 10), "stereo": (6, 10)},
}

# the `return` statements of each reference body, in source order
RETURNS = {"fuse": ("depth", "bounds", "distance", "viewing", "empty", "final"),
           "scw": ("depth", "depth", "bounds", "distance", "viewing", "empty", "final"),
           "sim3": ("depth", "bounds", "distance", "empty", "final"),
           "fkf": ("bounds", "distance", "empty", "final"),
           "local": ("depth", "bounds", "bounds", "distance", "viewing", "final")}
BODY = {"fuse": O.single_item, "scw": SO.single_item, "sim3": S3.single_item, "fkf": FK.single_item,
        "local": LO.frustum_one}


def _return_lines(fn):
    return [i for i, line in enumerate(inspect.getsource(fn).splitlines()) if line.strip().startswith("return")]


_LINES = {m: _return_lines(fn) for m, fn in BODY.items()}
assert all(len(_LINES[m]) == len(RETURNS[m]) for m in MODES), {m: len(_LINES[m]) for m in MODES}
_FUNCS = list(BODY.values()) + [LO.fp_one, MW.KeyFrame.get_features_in_area, MW.Frame.get_features_in_area,
                                MW.MapPoint.predict_scale]
_TRACED = {fn.__code__: set(_return_lines(fn)) for fn in _FUNCS}
_KEEP = ("x0", "x1", "y0", "y1", "r", "out", "best_idx", "best_dist", "best_dist2", "best_level2")


def traced(fn, *args):
    """fn(*args) and what each traced function returned by: [(name, line of the `return` statement within the
    function, value, locals)].  The line is the last `return` statement the frame came to: a return out of a `with`
    block passes the `with` line once more."""
    events, last = [], {}

    def local(frame, event, arg):
        co = frame.f_code
        if event == "line":
            if frame.f_lineno - co.co_firstlineno in _TRACED[co]:
                last[id(frame)] = frame.f_lineno - co.co_firstlineno
        elif event == "return":
            loc = frame.f_locals
            events.append((co.co_name, last.pop(id(frame), -1), arg, {k: loc[k] for k in _KEEP if k in loc}))
        return local

    def call(frame, event, arg):
        return local if frame.f_code in _TRACED else None
    old = sys.gettrace()
    sys.settrace(call)
    try:
        res = fn(*args)
    finally:
        sys.settrace(old)
    return res, events


def local_reference(F, p, limit, th):
    """Frame.is_in_frustum and, for a point in view, the body of search_by_projection_f_p on the stand-in objects, in
    the array oracle's terms: ((in_view, level, winner, distance, the second's octave, the second's distance), the
    trace).  The reference keeps the second candidate's distance and octave, not its index; the frame's slots are put
    back."""
    seen, ev = traced(LO.frustum_one, F, p, limit)
    if not seen:
        return (0, -1, -1, -1, -1, -1), ev
    slots = list(F.mvpMapPoints)
    _, ev2 = traced(LO.fp_one, F, p, th, 1.0)
    F.mvpMapPoints = slots
    loc = ev2[-1][3]
    bd, bd2 = loc.get("best_dist", 256), loc.get("best_dist2", 256)
    return (1, int(p.mnTrackScaleLevel), int(loc.get("best_idx", -1)), -1 if bd == 256 else int(bd),
            int(loc.get("best_level2", -1)), -1 if bd2 == 256 else int(bd2)), ev + ev2


# ---- neighbours of a float ------------------------------------------------------------------------------------------

def _ordinal(x, dtype):
    """An integer that grows with x over the dtype's representable values, adjacent values one apart."""
    it, mask = (np.int32, (1 << 31) - 1) if dtype == np.float32 else (np.int64, (1 << 63) - 1)
    i = int(np.array(x, dtype).view(it))
    return i if i >= 0 else -(i & mask)


def _value(o, dtype):
    it, bits = (np.int32, 31) if dtype == np.float32 else (np.int64, 63)
    return np.array(o if o >= 0 else -o - (1 << bits), it).view(dtype)[()]


def bisect(pred, lo, hi, dtype):
    """Ordinals (a, b), one apart, with pred(a) == pred(lo) != pred(b), between lo and hi."""
    a, b = _ordinal(lo, dtype), _ordinal(hi, dtype)
    pa = pred(_value(a, dtype))
    if pred(_value(b, dtype)) == pa:
        return None
    while abs(b - a) > 1:
        m = (a + b) // 2
        if pred(_value(m, dtype)) == pa:
            a = m
        else:
            b = m
    return a, b


# ---- the worlds ------------------------------------------------------------------------------------------------------

def _pose(rng, t=0.5, r=0.03):
    """A pose of a small rotation, from a quaternion: only + - * / and sqrt, and uniform draws, so every machine
    builds the same world to the last bit."""
    a, b, c = (float(x) for x in rng.uniform(-r, r, 3))
    n = math.sqrt(1.0 + a * a + b * b + c * c)
    w, x, y, z = 1.0 / n, a / n, b / n, c / n
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.uniform(-t, t, 3)
    return T


def _apply(R, v):
    """R v for a 3 x 3 R, term by term in a fixed order (no BLAS)."""
    return np.array([(R[r][0] * v[0] + R[r][1] * v[1]) + R[r][2] * v[2] for r in range(3)])


def _inverse(A):
    """The inverse of a 3 x 3 matrix by cofactors."""
    a, b, c = A[0], A[1], A[2]
    co = np.array([np.cross(b, c), np.cross(c, a), np.cross(a, b)])
    return co.T / float(np.dot(a, np.cross(b, c)))


STEP_Z = 1.3593563908785256        # 100 ^ (1 / 15): the depths go over a factor of 100 in START - 1 steps
BELOW = 0.946772480999074          # 1.2 ^ -0.3


def _power(b, n):
    out = 1.0
    for _ in range(n):
        out *= b
    return out


US, VS, LEVELS = (45.0, 255.0, 615.0, 930.0, 1195.0), (32.0, 188.0, 343.0), (0, 1, 4, 7)


class Start:
    """A start item: a map point placed to project to (u, v) at depth z in target k and to predict level L there."""


class Set:
    """The world and the ladders of one (mode, precision)."""

    def __init__(self, mode, prec, j_max=J):
        self.mode, self.prec, self.dtype, self.eps, self.j_max = mode, prec, DTYPE[prec], EPS[prec], j_max
        self.th = TH_LOCAL[prec] if mode == "local" else TH[mode]
        rng = np.random.Generator(np.random.PCG64(1000 * MODES.index(mode) + 7 * PRECISIONS.index(prec) + 3))
        self.world = MW.World()
        self.targets, self.ctx, self.starts = [], [], []
        for k in range(2):
            self._target(rng, k)
        self.ladders = []
        for gate in GATES[mode]:
            self._gate(gate)

    # -- construction
    def _chain(self, rng, k):
        """What the mode's body gets besides the target and the point, and camera -> world and the camera centre in
        float64 for placing the start items."""
        dt, mode = self.dtype, self.mode
        T = _pose(rng)
        if mode == "scw":
            S = MW.sim3(T, (1.3, 0.8)[k]).astype(dt)
            pose = SO.fuse_pose(S)
            R, t = pose[0].astype(np.float64), pose[1].astype(np.float64).reshape(3)
            return dict(T=T.astype(dt), Scw=S, pose=pose), (lambda pc: _apply(R.T, pc - t)), -_apply(R.T, t)
        if mode == "sim3":
            # the parts search_by_sim3 derives from (pKF1's pose, s12, R12, t12), by the reference's expressions: the
            # point goes through pKF1's pose and then through (sR21, t21), whose scale is 1 / s12
            Tw, Trel, s = _pose(rng).astype(dt), _pose(rng), SIM3_SCALES[k]
            s12, R12, t12 = 1.0 / s, Trel[:3, :3].astype(dt), Trel[:3, 3:4].astype(dt)
            _, sR, t = S3.sim3_parts(s12, R12, t12)
            Rw, tw = Tw[:3, :3].copy(), Tw[:3, 3:4].copy()
            assert sR.dtype == t.dtype == dt
            A, a, B, b = (x.astype(np.float64) for x in (Rw, tw.reshape(3), sR, t.reshape(3)))
            Bi = _inverse(B)
            return (dict(T=T.astype(dt), Tw=Tw, Rw=Rw, tw=tw, sR=sR, t=t, s=s, s12=s12, R12=R12, t12=t12),
                    (lambda pc: _apply(A.T, _apply(Bi, pc - b) - a)), None)
        Td = T.astype(dt)
        R, t = Td[:3, :3].astype(np.float64), Td[:3, 3].astype(np.float64)
        return dict(T=Td), (lambda pc: _apply(R.T, pc - t)), -_apply(R.T, t)

    def _target(self, rng, k):
        mode, dt = self.mode, self.dtype
        ctx, to_world, Ow = self._chain(rng, k)
        n = 2 * START + 6
        a = MW.kf_arrays(rng, n)
        a["uR"][:] = -1.0
        first = len(self.starts)
        for i in range(START):
            s = Start()
            s.k, s.i, s.home = k, first + i, 2 * i
            s.u = US[(i + 2 * k) % 5] + float(rng.uniform(-8, 8))
            s.v = VS[i % 3] + float(rng.uniform(-6, 6))
            if mode in ("fkf", "local"):
                # a frame's window truncates at both ends while its grid rounds: a quarter into its cell, the start
                # item's own feature lies in a cell that the window visits
                cw, ch = MW.W / MW.GRID_COLS, MW.H / MW.GRID_ROWS
                s.u, s.v = (math.floor(s.u / cw) + 0.25) * cw, (math.floor(s.v / ch) + 0.28) * ch
            s.z = 1.5 * _power(STEP_Z, (5 * i) % START) * float(rng.uniform(0.9, 1.1))
            s.L = LEVELS[(i + k) % 4]
            s.per = 1.0 / ctx.get("s", 1.0)         # a step in the world per step in the target camera
            pc = np.array([(s.u - MW.CX) * s.z / MW.FX, (s.v - MW.CY) * s.z / MW.FY, s.z])
            s.pos = to_world(pc).astype(dt)
            po = pc if Ow is None else s.pos.astype(np.float64) - Ow
            s.dist = math.sqrt(float((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2]))
            s.nrm = (po / s.dist).astype(dt)
            s.max_d = s.dist * _power(1.2, s.L) * BELOW    # the quotient is L - 0.3: level L with room on both sides
            s.min_d = s.dist / (1.3 * 0.8)                 # the minimum distance is dist / 1.3
            sc = MW.SF[s.L]
            s.r = sc * (2.5 * (self.th if self.th != 1.0 else 1.0) if mode == "local" else self.th)
            s.desc = rng.integers(0, 256, 32, dtype=np.uint8)
            ur = s.u - MW.BF / s.z
            h, tw = s.home, s.home + 1
            a["x"][h], a["y"][h], a["octave"][h] = s.u + 0.6 * sc, s.v - 0.45 * sc, s.L
            a["desc"][h] = MW.noisy_desc(rng, s.desc, 3)
            if mode == "local":
                s.stereo = i % 8 != 7 and ur + 0.55 * s.r > 1.0
                a["uR"][h] = ur + 0.55 * s.r if s.stereo else -1.0
            else:
                s.stereo = i % 2 == 0 and ur + 0.3 >= 0.0
                a["uR"][h] = ur + 0.3 if s.stereo else -1.0
            a["x"][tw], a["y"][tw], a["octave"][tw] = s.u - 0.5 * sc, s.v + 0.3 * sc, s.L
            a["desc"][tw] = MW.noisy_desc(rng, s.desc, 40)
            self.starts.append(s)
        T = ctx["T"]
        if mode == "fkf":
            tg = KC.Frame(self.world, a, T)
            tg.Tcw = tg.mTcw = T
        elif mode == "local":
            tg = LC.Frame(self.world, a, T, mn_id=40 + k)
        else:
            tg = MW.KeyFrame(self.world, k, a, T)
            tg.Tcw = T
        self.targets.append(tg)
        self.ctx.append(ctx)

    def point(self, s, scalar=None, value=None, mid=None):
        """The start item's map point, with one scalar replaced by a value of its own dtype."""
        pos, nrm = s.pos.copy(), s.nrm.copy()
        if scalar is not None:
            (pos if scalar[0] == "p" else nrm)[int(scalar[1])] = value
        cls = LC.MapPoint if self.mode == "local" else MW.MapPoint
        p = cls(self.world, s.i if mid is None else mid, pos, s.desc, nrm, s.min_d, s.max_d)
        p._pos, p._normal = pos.reshape(3, 1), nrm.reshape(3, 1)
        assert p._pos.dtype == p._normal.dtype == self.dtype
        return p

    def first_keyframe(self, k, pts):
        """pKF1 of search_by_sim3 for target k: the pose the ladders went through, and one feature slot per point."""
        rng = np.random.Generator(np.random.PCG64(5 + k))
        kf = MW.KeyFrame(self.world, 10 + k, MW.kf_arrays(rng, len(pts)), self.ctx[k]["Tw"])
        kf.Tcw = self.ctx[k]["Tw"]
        kf.mvpMapPoints = list(pts)
        return kf

    # -- the reference body
    def reference(self, k, p):
        """(what the reference body decides for point p in target k, in the array oracle's terms; its trace).
        fuse, scw, sim3, fkf: (winner, distance), -1 for none.  local: (in_view, level, winner, distance, the second's
        octave, the second's distance)."""
        tg, c, mode = self.targets[k], self.ctx[k], self.mode
        if mode == "local":
            return local_reference(tg, p, LIMIT, self.th)
        if mode == "fuse":
            (dist, idx), ev = traced(O.single_item, tg, p, self.th)
        elif mode == "scw":
            (dist, idx), ev = traced(SO.single_item, tg, p, c["pose"], self.th, None)
        elif mode == "sim3":
            (dist, idx), ev = traced(S3.single_item, p, c["Rw"], c["tw"], c["sR"], c["t"], tg, self.th,
                                     (tg.fx, tg.fy, tg.cx, tg.cy))
        else:
            (dist, idx), ev = traced(FK.single_item, tg, p, self.th)
        return (int(idx), int(dist) if idx >= 0 else -1), ev

    def decision(self, gate, sub, s, out, ev):
        """The reference body's decision at one gate, from its result and trace."""
        body = BODY[self.mode].__name__
        left = next(RETURNS[self.mode][_LINES[self.mode].index(e[1])] for e in ev if e[0] == body)
        area = next((e[3] for e in ev if e[0] == "get_features_in_area"), None)
        if gate in ("depth", "bounds", "distance", "viewing"):
            return left == gate
        if gate == "level":
            return next((e[2] for e in ev if e[0] == "predict_scale"), None)
        if gate == "radius":
            return next((e[3].get("r") for e in ev if e[0] == "fp_one"), None)
        if gate == "window":
            return None if area is None else area.get(sub)
        if gate == "candidate":
            return area is not None and s.home in area.get("out", ())
        if gate in ("chi-square", "stereo"):
            return (out[2] if self.mode == "local" else out[0]) == s.home
        raise KeyError(gate)

    # -- the ladders
    def _plans(self, gate):
        """Candidate (sub, start, scalar, far value) in order of preference; the first N_LADDERS that flip are kept,
        as evenly over the subs as they come."""
        S, fx, fy = self.starts, MW.FX, MW.FY
        wide = [s for s in S if abs(s.u - MW.CX) >= 150]     # |p0| is no smaller than the terms it is summed with
        tall = [s for s in S if abs(s.v - MW.CY) >= 100]
        plans = []
        if gate == "depth":
            # where zc passes 0, p2 is about the camera centre's: small beside the lateral terms of a far, off-centre point
            plans = [("zc", s, "p2", s.pos[2] - 3 * s.z)
                     for s in sorted(S, key=lambda s: s.z * (abs(s.u - MW.CX) + abs(s.v - MW.CY)))]
        elif gate == "bounds":
            for sub, key, sc, sign, f, span in (("minX", "u", "p0", -1, fx, MW.W), ("maxX", "u", "p0", 1, fx, MW.W),
                                                ("minY", "v", "p1", -1, fy, MW.H), ("maxY", "v", "p1", 1, fy, MW.H)):
                near = sorted(S, key=lambda s: sign * -getattr(s, key))
                plans += [(sub, s, sc, s.pos[int(sc[1])] + sign * 1.3 * span * s.z / f) for s in near[:8]]
        elif gate == "distance":
            plans = [("min", s, "p2", s.pos[2] - 0.5 * s.z) for s in S if abs(s.u - MW.CX) < 400]
            plans += [("max", s, "p2", s.pos[2] + 2.0 * s.z) for s in S if s.L <= 1]
        elif gate == "viewing":
            plans = [("cos", s, "n2", s.nrm[2] - 2.0) for s in S if abs(s.u - MW.CX) < 400]   # n2 stays near 0.5
        elif gate == "radius":
            plans = [("0.998", s, "n2", s.nrm[2] - 0.2) for s in S]
        elif gate == "level":
            for s in S:
                if s.L == 0:
                    plans.append(("0|1", s, "p2", s.pos[2] - 0.2 * s.z))
                else:
                    plans.append(({1: "0|1", 7: "top-1|top"}.get(s.L, "inner"), s, "p2", s.pos[2] + 0.45 * s.z))
        elif gate == "window":
            cw, ch = MW.W / MW.GRID_COLS, MW.H / MW.GRID_ROWS
            for sub, pool, sc, key, c, cell, f in (("x0", wide, "p0", "u", MW.CX, cw, fx), ("x1", wide, "p0", "u", MW.CX, cw, fx),
                                                   ("y0", tall, "p1", "v", MW.CY, ch, fy), ("y1", tall, "p1", "v", MW.CY, ch, fy)):
                for s in pool:
                    inward = -1.0 if getattr(s, key) > c else 1.0
                    plans.append((sub, s, sc, s.pos[int(sc[1])] + inward * 1.2 * cell * s.z / f))
        elif gate == "candidate":
            plans = [("dx", s, "p0", s.pos[0] - 1.5 * s.r * s.z / fx) for s in wide]
            plans += [("dy", s, "p1", s.pos[1] + 1.5 * s.r * s.z / fy) for s in tall]
        elif gate == "chi-square":
            plans = [("7.8" if s.stereo else "5.99", s, "p0", s.pos[0] - 1.2 * s.r * s.z / fx) for s in wide]
        elif gate == "stereo":
            plans = [("uR", s, "p0", s.pos[0] - 0.9 * s.r * s.z / fx)
                     for s in sorted(S, key=lambda s: -abs(s.u - MW.CX)) if s.stereo]
        return plans

    def _gate(self, gate):
        dt = self.dtype
        found = {}
        for sub, s, scalar, far in self._plans(gate):
            if scalar[0] == "p":
                far = s.pos[int(scalar[1])] + (far - s.pos[int(scalar[1])]) * s.per
            def dec(v, s=s, scalar=scalar, sub=sub):
                out, ev = self.reference(s.k, self.point(s, scalar, v))
                return self.decision(gate, sub, s, out, ev)
            here = (s.pos if scalar[0] == "p" else s.nrm)[int(scalar[1])]
            d0 = dec(here)
            if d0 is None:
                continue
            ab = bisect(lambda v: dec(v) == d0, here, dt(far), dt)
            if ab is None:
                continue
            a, b = ab
            if dec(_value(b, dt)) is None and gate in ("level", "window", "radius"):
                continue   # another gate took the item away first: not this gate's flip
            if scalar[0] == "p" and gate != "depth":
                # the units of a scalar that has all but cancelled against the terms it is summed with (the other
                # coordinates and the translations, about half a unit of the target's each) are far below the
                # bound's: such a ladder would need many more rungs than the others
                others = sum(abs(float(x)) for x in s.pos) + 0.5 * (1.0 + s.per)
                if abs(float(_value(a, dt))) < 0.1 * others:
                    continue
            step = 1 if b > a else -1
            rungs = []
            for j in range(self.j_max + 1):
                rungs.append((-(1 << j), _value(a - step * ((1 << j) - 1), dt)))
                rungs.append(((1 << j), _value(b + step * ((1 << j) - 1), dt)))
            found.setdefault(sub, []).append(dict(mode=self.mode, prec=self.prec, gate=gate, sub=sub, start=s,
                                                  scalar=scalar, rungs=sorted(rungs, key=lambda r: r[0])))
        if gate == "depth":
            # where zc passes 0 the scalar has cancelled against the other terms of the sum (the other coordinates and
            # the translations, about half a unit of the target's each); the ladders whose scalar is largest beside
            # those terms step in units nearest to the bound's own
            def share(lad):
                s0 = lad["start"]
                v = abs(float(lad["rungs"][len(lad["rungs"]) // 2][1]))
                return v / (v + abs(float(s0.pos[0])) + abs(float(s0.pos[1])) + 0.5 * (1.0 + s0.per))
            for lads in found.values():
                lads.sort(key=lambda lad: -share(lad))
        # as evenly over the subs as they come
        keep, subs = [], sorted(found)
        while len(keep) < N_LADDERS and any(found[x] for x in subs):
            for x in subs:
                if found[x] and len(keep) < N_LADDERS:
                    keep.append(found[x].pop(0))
        assert len(keep) == N_LADDERS, (self.mode, self.prec, gate, len(keep))
        self.ladders += keep

    # -- the arrays
    def items(self):
        """[(ladder index, rung label, target, map point)] in the order of the point table; a point's mnId is its
        place in it."""
        flat = [(n, lab, lad, v) for n, lad in enumerate(self.ladders) for lab, v in lad["rungs"]]
        return [(n, lab, lad["start"].k, self.point(lad["start"], lad["scalar"], v, mid))
                for mid, (n, lab, lad, v) in enumerate(flat)]

    def arrays(self, items, device=False):
        """(the entry's arrays over the items, per item its index into the flat outputs).  device: without the rungs
        whose level quotient is within Q_GUARD of an integer (there the device's log may round the other way)."""
        mode, tg = self.mode, self.targets
        pts = [it[3] for it in items]
        if mode in ("fuse", "scw"):
            a = O.pack(tg, pts, self.th) if mode == "fuse" else SO.pack(tg, [c["Scw"] for c in self.ctx], pts, self.th)
            at = [it[2] * len(pts) + n for n, it in enumerate(items)]
        else:
            lists = [[n for n, it in enumerate(items) if it[2] == k] for k in range(2)]
            at = {n: i for i, n in enumerate(lists[0] + lists[1])}
            at = [at[n] for n in range(len(items))]
            if mode == "sim3":
                rows = [O.pack_point(p) for p in pts]
                srch = [S3.srch_row((t.fx, t.fy, t.cx, t.cy), c["Rw"], c["tw"], c["sR"], c["t"])
                        for t, c in zip(tg, self.ctx)]
                a = S3.join([O.pack_kf(t) for t in tg], [r[0] for r in rows], [r[1] for r in rows], srch, [0, 1],
                            lists, self.th, self.eps)
            elif mode == "fkf":
                rows = [FK.pack_point(p) for p in pts]
                a = FK.join([FK.pack_frame(t) for t in tg], [np.zeros(t.N, np.uint8) for t in tg],
                            [r[0] for r in rows], [r[1] for r in rows], [0, 1], lists, self.th, self.eps)
            else:
                rows = [O.pack_point(p) for p in pts]
                a = LO.join([LO.pack_frame(t) for t in tg], [np.zeros(t.N, np.uint8) for t in tg],
                            [r[0] for r in rows], [r[1] for r in rows], [LIMIT, LIMIT], [0, 1], lists, self.th,
                            self.th != 1.0, self.eps)
        assert a["eps"] == self.eps
        return a, at

    def oracle_item(self, a, items, at, n):
        """The array oracle's outputs for item n alone, status last."""
        k = items[n][2]
        if self.mode == "fuse":
            return O.search_item(a, k, n)
        if self.mode == "scw":
            return SO.search_item(a, k, n)
        return {"sim3": S3.search_item, "fkf": FK.search_item, "local": LO.search_item}[self.mode](a, k, at[n])

    def search(self, a):
        return {"fuse": O.search, "scw": SO.search, "sim3": S3.search, "fkf": FK.search, "local": LO.search}[self.mode](a)

    def quotient(self, a, items, n):
        """The level quotient log(maxD / dist) / lsf of item n in the kernel's own operations and order, so it is
        the array oracle's bit for bit."""
        k = items[n][2]
        K, P = [float(x) for x in a["kf_f64"][k]], [float(x) for x in a["pt_f64"][n]]
        if self.mode == "sim3":
            S = [float(x) for x in a["srch_f64"][k]]
            Rw, tw, sR, t = S[4:13], S[13:16], S[16:25], S[25:28]
            c = [((Rw[3 * r] * P[0] + Rw[3 * r + 1] * P[1]) + Rw[3 * r + 2] * P[2]) + tw[r] for r in range(3)]
            x = [((sR[3 * r] * c[0] + sR[3 * r + 1] * c[1]) + sR[3 * r + 2] * c[2]) + t[r] for r in range(3)]
        else:
            x = [P[r] - K[17 + r] for r in range(3)]
        dist = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        return O._div(O._log(O._div(P[8], dist)), K[26])


def evaluate(S):
    """Everything the tests ask of a set, computed once: per item the array oracle's outputs, the reference body's,
    the reference's decision at the ladder's gate and the level quotient."""
    if getattr(S, "_eval", None) is None:
        items = S.items()
        a, at = S.arrays(items)
        got, ref, dec, quo = [], [], [], []
        for n, (lad, _, k, p) in enumerate(items):
            L = S.ladders[lad]
            got.append(tuple(int(x) for x in S.oracle_item(a, items, at, n)))
            out, ev = S.reference(k, p)
            ref.append(out)
            dec.append(S.decision(L["gate"], L["sub"], L["start"], out, ev))
            quo.append(S.quotient(a, items, n))
        S._eval = dict(items=items, a=a, at=at, got=got, ref=ref, dec=dec, quo=quo)
    return S._eval


def ladder_rungs(S, li):
    """{rung label: item index} of ladder li."""
    E = evaluate(S)
    return {it[1]: n for n, it in enumerate(E["items"]) if it[0] == li}


def marked(S, n):
    return evaluate(S)["got"][n][-1] != 0


def is_closed(S, li):
    """A ladder is closed if its two outermost rungs are unmarked."""
    r = ladder_rungs(S, li)
    return not marked(S, r[-(1 << S.j_max)]) and not marked(S, r[1 << S.j_max])


def mark_ends_at(S, li):
    """The smallest j from which on the rungs +-2^j .. +-2^J are all unmarked: where the mark disappears, which pins
    the bound's size to a factor of two.  None for an open ladder."""
    r = ladder_rungs(S, li)
    j = S.j_max + 1
    while j > 0 and not marked(S, r[-(1 << (j - 1))]) and not marked(S, r[1 << (j - 1)]):
        j -= 1
    return j if j <= S.j_max else None


def signature(S, k, p):
    """Everything the reference body decided for a point, gate by gate: the `return`s it left by, the level, the
    window, the candidates, the radii and the result."""
    out, ev = S.reference(k, p)
    return tuple((e[0], e[1], e[2] if e[0] == "predict_scale" else None,
                  tuple(sorted((a, tuple(b) if isinstance(b, list) else float(np.asarray(b).reshape(-1)[0]))
                               for a, b in e[3].items()))) for e in ev) + (out,)


def neighbour_of(S, li, reach=3):
    """For an open ladder: the other decision of the reference body that also changes near the flip, looked for up
    to 2^(J + reach) units on either side, as the name of the traced function whose outcome changes; None if the
    reference decides the same all the way on both sides."""
    lad = S.ladders[li]
    s, dt = lad["start"], S.dtype
    lo, hi = lad["rungs"][len(lad["rungs"]) // 2 - 1][1], lad["rungs"][len(lad["rungs"]) // 2][1]
    a, b = _ordinal(lo, dt), _ordinal(hi, dt)
    step = 1 if b > a else -1
    for base, sign in ((a, -step), (b, step)):
        first = signature(S, s.k, S.point(s, lad["scalar"], _value(base, dt)))
        for j in range(S.j_max + reach + 1):
            sig = signature(S, s.k, S.point(s, lad["scalar"], _value(base + sign * ((1 << j) - 1), dt)))
            if sig != first:
                return next((x[0] for x, y in zip(sig, first) if x != y and isinstance(x, tuple) and len(x) == 4), "result")
    return None


def device_rungs(S):
    """The items that go to a device: all but those whose level quotient lies within Q_GUARD of an integer, where
    ceil() of the device's log may differ from NumPy's.  (items, the indices left out)."""
    E = evaluate(S)
    out = [n for n, q in enumerate(E["quo"]) if math.isfinite(q) and abs(q - round(q)) < Q_GUARD]
    drop = set(out)
    return [it for n, it in enumerate(E["items"]) if n not in drop], out


def groups(S):
    """{gate: [ladder indices]}; the Sim3 search's "two-stage pose" is every one of its ladders."""
    g = {}
    for li, lad in enumerate(S.ladders):
        g.setdefault(lad["gate"], []).append(li)
    if S.mode == "sim3":
        g["two-stage pose"] = list(range(len(S.ladders)))
    return g


def same_as_reference(mode, got, ref, octave_of):
    """Whether the array oracle's outputs of an item (status last) are what the reference body decided.  local: the
    reference keeps the second candidate's distance and octave, not its index."""
    if mode != "local":
        return tuple(int(x) for x in got[:2]) == ref
    in_view, level, bi, bd, si, sd = (int(x) for x in got[:6])
    if not in_view:
        return ref[0] == 0
    return (in_view, level, bi, bd, octave_of(si) if si >= 0 else -1, sd) == ref


_SETS = {}


def get(mode, prec):
    """The set of a (mode, precision), built once and shared; nobody changes it."""
    if (mode, prec) not in _SETS:
        _SETS[mode, prec] = Set(mode, prec)
    return _SETS[mode, prec]
