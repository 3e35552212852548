"""NumPy / Python restatement of k_local_search (include/orbfe.h, orbfe_local_search) over the entry's own arrays, for
the tests: Frame.is_in_frustum (Frame.py:328-371) and the search half of ORBMatcher.search_by_projection_f_p
(ORBMatcher.py:215-283, with Frame.get_features_in_area, Frame.py:373-416) in float64 with the error bounds and the
ORBFE_FUSE_MARGINAL bit of the device, operation for operation.  A search is a target frame, a limit of the viewing
cosine and a list of rows of one shared point table; a frame carries one blocked byte and one right coordinate per
feature.

The switches of `geometry` / `search_item` exist for the non-vacuity tests only; each turns one property of the mode off:
    depth_gate       False: pc.z < 0 goes on, as in k_fkf_search
    stereo_gate      False: u_right is not looked at
    three_octaves    a candidate's octave lies in [level - 1, level + 1], as in k_fkf_search
    blocked          False: the blocked bytes are not looked at

Also the reference's two bodies on the stand-in objects of tests/local_search_cases.py (what a marked or overtaken
item is redone with), the packing of such objects into the arrays, and the whole Tracking.search_local_points from array
results (`replay`).
"""
from __future__ import annotations

import math

import numpy as np

import fkf_oracle as FK
import fuse_oracle as O
from fuse_oracle import _div, _isfinite, _log, _near_int

MARGINAL, KF_F64, PT_F64 = O.MARGINAL, O.KF_F64, O.PT_F64
EPS_F32, EPS_F64 = O.EPS_F32, O.EPS_F64
TH_HIGH = 100

KF_ARRAYS = ("kf_f64", "kf_i32", "off", "xy", "octave", "u_right", "desc", "blocked", "cell_at", "cell_off", "idx_at",
             "cell_idx", "lvl_off", "scale")
ARRAYS = KF_ARRAYS + ("pt_f64", "pt_desc", "srch_limit", "srch_kf", "srch_off", "item_pt")
OUTPUTS = ("in_view", "level", "best_idx", "best_dist", "second_idx", "second_dist", "status")


def geometry(K, ki, scale, P, limit, th, th_on, eps, depth_gate=True):
    """Phase 1 of the kernel for one item: (status, level, window).  level is -1 when the item is not in view;
    window is None when the item does not reach the candidates, else (u, v, ur, Eu, Ev, Eur, r, x0, x1, y0, y1, vc)."""
    K, P = [float(x) for x in K], [float(x) for x in P]
    cols, rows, levels = (int(x) for x in ki)
    fx, fy, cx, cy, bf = K[0:5]
    minX, maxX, minY, maxY, winv, hinv, lsf = K[20:27]
    p0, p1, p2 = P[0:3]
    f = np.float64
    with np.errstate(all="ignore"):
        xc = float(((f(K[5]) * p0 + f(K[6]) * p1) + f(K[7]) * p2) + K[14])
        yc = float(((f(K[8]) * p0 + f(K[9]) * p1) + f(K[10]) * p2) + K[15])
        zc = float(((f(K[11]) * p0 + f(K[12]) * p1) + f(K[13]) * p2) + K[16])
        Ex = float(4.0 * eps * (((abs(f(K[5]) * p0) + abs(f(K[6]) * p1)) + abs(f(K[7]) * p2)) + abs(K[14])))
        Ey = float(4.0 * eps * (((abs(f(K[8]) * p0) + abs(f(K[9]) * p1)) + abs(f(K[10]) * p2)) + abs(K[15])))
        Ez = float(4.0 * eps * (((abs(f(K[11]) * p0) + abs(f(K[12]) * p1)) + abs(f(K[13]) * p2)) + abs(K[16])))
    st = 0
    if depth_gate and zc < 0.0:
        return (MARGINAL if -zc < Ez else 0), -1, None
    if zc < Ez:
        st = MARGINAL
    if zc == 0.0:
        return MARGINAL, -1, None
    with np.errstate(all="ignore"):
        iz = _div(1.0, zc)
        aiz = abs(iz)
        xn, yn = float(f(fx) * xc), float(f(fy) * yc)
        fxx, fyy = float(f(xn) * iz), float(f(yn) * iz)
        u, v = float(f(fxx) + cx), float(f(fyy) + cy)
        bz = float(f(bf) * iz)
        ur = float(f(u) - bz)
        rz = _div(Ez, abs(zc))
        if not rz <= 0.25:
            st = MARGINAL
        Eiz = float(f(aiz) * (f(2.0) * rz + 2.0 * eps))
        Ax, Ay = float(f(abs(fx)) * Ex), float(f(abs(fy)) * Ey)
        Exn = float(f(Ax) + f(eps) * (f(abs(xn)) + Ax))
        Eyn = float(f(Ay) + f(eps) * (f(abs(yn)) + Ay))
        Mu, Mv = float(f(abs(fxx)) + abs(cx)), float(f(abs(fyy)) + abs(cy))
        Bx = float(f(abs(xn)) * Eiz + f(Exn) * (f(aiz) + Eiz))
        By = float(f(abs(yn)) * Eiz + f(Eyn) * (f(aiz) + Eiz))
        Eu = float((f(Bx) + f(eps) * (f(abs(fxx)) + Bx)) + f(4.0 * eps) * Mu)
        Ev = float((f(By) + f(eps) * (f(abs(fyy)) + By)) + f(4.0 * eps) * Mv)
        Eur = float((f(Eu) + f(abs(bf)) * Eiz) + f(4.0 * eps) * (f(abs(bz)) + Mu))
        tot = float(((((f(u) + v) + ur) + Eu) + Ev) + Eur)
    if not _isfinite(tot):
        return MARGINAL, -1, None
    if (abs(u - minX) < Eu + eps * abs(minX) or abs(u - maxX) < Eu + eps * abs(maxX)
            or abs(v - minY) < Ev + eps * abs(minY) or abs(v - maxY) < Ev + eps * abs(maxY)):
        st = MARGINAL
    if u < minX or u > maxX or v < minY or v > maxY:
        return st, -1, None
    po0, po1, po2 = p0 - K[17], p1 - K[18], p2 - K[19]
    with np.errstate(all="ignore"):
        dist = float(np.sqrt(f((f(po0) * po0 + f(po1) * po1) + f(po2) * po2)))
    Ed = 6.0 * eps * dist
    minD, maxD = P[6], P[7]
    if not _isfinite(dist):
        return MARGINAL, -1, None
    if abs(dist - minD) < Ed + eps * abs(minD) or abs(dist - maxD) < Ed + eps * abs(maxD):
        st = MARGINAL
    if dist < minD or dist > maxD:
        return st, -1, None
    with np.errstate(all="ignore"):
        t0, t1, t2 = float(f(po0) * P[3]), float(f(po1) * P[4]), float(f(po2) * P[5])
        dot = float((f(t0) + t1) + t2)
        vc = _div(dot, dist)
        Evc = float(_div(float(f(5.0 * eps) * ((f(abs(t0)) + abs(t1)) + abs(t2))), dist) + f(8.0 * eps) * abs(vc))
    if not _isfinite(vc + Evc):
        return MARGINAL, -1, None
    if abs(vc - limit) < Evc + eps * abs(limit) or abs(vc - 0.998) < Evc + eps * 0.998:
        st = MARGINAL
    if vc < limit:
        return st, -1, None
    q = _div(_log(_div(P[8], dist)), lsf)
    if not _isfinite(q):
        return MARGINAL, -1, None
    if _near_int(q, _div(10.0 * eps, abs(lsf)) + 4.0 * eps * abs(q)):
        st = MARGINAL
    cq = math.ceil(q)
    level = 0 if cq < 0 else (levels - 1 if cq > levels - 1 else int(cq))
    r0 = 2.5 if vc > 0.998 else 4.0
    with np.errstate(all="ignore"):
        if th_on:
            r0 = float(f(r0) * th)
        r = float(f(r0) * float(scale[level]))
        ax, bx = float((f(u - minX) - r) * winv), float((f(u - minX) + r) * winv)
        ay, by = float((f(v - minY) - r) * hinv), float((f(v - minY) + r) * hinv)
        tot = float((f(ax) + bx) + (f(ay) + by))
    if not _isfinite(tot):
        return MARGINAL, level, None
    Ewx = abs(winv) * (Eu + 4.0 * eps * ((abs(u) + abs(minX)) + abs(r)))
    Ewy = abs(hinv) * (Ev + 4.0 * eps * ((abs(v) + abs(minY)) + abs(r)))
    # int() truncates toward zero: (-1, 1) is cell 0, so only an integer of magnitude >= 1 separates two outcomes
    if any(abs(a) > 0.5 and _near_int(a, E) for a, E in ((ax, Ewx), (bx, Ewx), (ay, Ewy), (by, Ewy))):
        st = MARGINAL
    lo_x, hi_x, lo_y, hi_y = math.trunc(ax), math.trunc(bx), math.trunc(ay), math.trunc(by)
    if lo_x >= cols or hi_x < 0 or lo_y >= rows or hi_y < 0:
        return st, level, None
    x0, x1 = max(0, lo_x), min(cols - 1, hi_x)
    y0, y1 = max(0, lo_y), min(rows - 1, hi_y)
    return st, level, (u, v, ur, Eu, Ev, Eur, r, x0, x1, y0, y1, vc)


search_of = FK.search_of


def _window(a, s, i, **kw):
    k = int(a["srch_kf"][s])
    lo = int(a["lvl_off"][k])
    ki = a["kf_i32"][k]
    row = int(a["item_pt"][i])
    return k, row, geometry(a["kf_f64"][k], ki, a["scale"][lo:lo + int(ki[2])], a["pt_f64"][row],
                            float(a["srch_limit"][s]), float(a["th"]), bool(a["th_on"]), a["eps"], **kw)


def candidates(a, s, i, stereo_gate=True, three_octaves=False, blocked=True, **kw):
    """(in_view, level, status, [(distance, position, feature)] in visiting order) of item i of search s."""
    eps = a["eps"]
    k, row, (st, level, g) = _window(a, s, i, **kw)
    if g is None:
        return int(level >= 0), level, st, []
    rows = int(a["kf_i32"][k][1])
    u, v, ur, Eu, Ev, Eur, r, x0, x1, y0, y1, _ = g
    base = int(a["off"][k])
    coff = a["cell_off"][int(a["cell_at"][k]):]
    cidx = a["cell_idx"][int(a["idx_at"][k]):]
    blk = a["blocked"] if blocked else None
    er_r = eps * abs(r)
    out = []
    for ix in range(x0, x1 + 1):
        for pos in range(int(coff[ix * rows + y0]), int(coff[ix * rows + y1 + 1])):
            f = int(cidx[pos])
            if blk is not None and blk[base + f]:
                continue
            kx, ky = float(a["xy"][base + f][0]), float(a["xy"][base + f][1])
            dx, dy = kx - u, ky - v
            Edx = Eu + 2.0 * eps * (abs(kx) + abs(u))
            Edy = Ev + 2.0 * eps * (abs(ky) + abs(v))
            if abs(abs(dx) - r) < Edx + er_r or abs(abs(dy) - r) < Edy + er_r:
                st = MARGINAL
            if not (abs(dx) < r and abs(dy) < r):
                continue
            o = int(a["octave"][base + f])
            if o < level - 1 or o > level + (1 if three_octaves else 0):
                continue
            kr = float(a["u_right"][base + f])
            if stereo_gate and kr > 0.0:
                er = abs(ur - kr)
                Eer = Eur + 2.0 * eps * (abs(kr) + abs(ur))
                if abs(er - r) < Eer + er_r:
                    st = MARGINAL
                if er > r:
                    continue
            out.append((O.popcount(a["desc"][base + f], a["pt_desc"][row]), pos, f))
    return 1, level, st, out


def search_item(a, s, i, **kw):
    """The seven outputs of item i, which belongs to search s, of the arrays `a` (the entry's arguments by name, plus
    th, th_on and eps).  The two smallest keys (distance, visiting position) are what the reference's sequential
    update holds after the last candidate."""
    in_view, level, st, cand = candidates(a, s, i, **kw)
    two = sorted(cand)[:2] + [(-1, -1, -1)] * 2
    return in_view, level, two[0][2], two[0][0], two[1][2], two[1][0], st


def sequential(cand):
    """The reference's update (ORBMatcher.py:266-274) over candidates in visiting order, with their features:
    (best_idx, best_dist, second_idx, second_dist), -1 for none."""
    best = second = (256, -1)
    for d, _, f in cand:
        if d < best[0]:
            best, second = (d, f), best
        elif d < second[0]:
            second = (d, f)
    return (best[1], best[0] if best[1] >= 0 else -1, second[1], second[0] if second[1] >= 0 else -1)


def search(a, **kw):
    """The seven outputs, flat over the items, in OUTPUTS' order."""
    off = [int(x) for x in a["srch_off"]]
    n = off[-1] if off else 0
    out = [np.zeros(n, np.uint8) if k in ("in_view", "status") else np.full(n, -1, np.int32) for k in OUTPUTS]
    for s in range(len(off) - 1):
        for i in range(off[s], off[s + 1]):
            for o, val in zip(out, search_item(a, s, i, **kw)):
                o[i] = val
    return tuple(out)


# ---- arrays --------------------------------------------------------------------------------------------------------

def join(frames, blocked, pt_f64, pt_desc, limits, srch_kf, items, th, th_on, eps):
    """The entry's arrays of frame dicts (pack_frame / fuse_cases.KfBuilder.build), one blocked array per frame (or
    None: nothing blocked anywhere), a point table and per search its limit, its target and its list of point rows."""
    b = FK.join(frames, blocked, pt_f64, pt_desc, srch_kf, items, th, eps)
    b["u_right"] = O.join(frames, pt_f64, pt_desc, th, eps)["u_right"]
    b["srch_limit"] = np.array(limits, np.float64).reshape(-1)
    b["th_on"] = bool(th_on)
    return b


def pack_frame(F):
    """A frame dict of the reference's Frame surface: fkf_oracle.pack_frame's with bf and the right coordinates."""
    d = FK.pack_frame(F)
    d["f64"][4] = F.mbf
    d["u_right"] = np.array([float(x) for x in F.mvuRight], np.float64)
    return d


def skipped(pMP, frame):
    """Tracking.search_local_points' two `continue`s (Tracking.py:446-449)."""
    return pMP.mnLastFrameSeen == frame.mnId or pMP.is_bad()


def pack(jobs, th, limit):
    """Arrays of search_local_points(F, vp, th, limit) for every (F, vp) of jobs (distinct frames), one search per
    job, every point the loop does not skip sent, and per search the list positions of its items."""
    frames, blocked, rows, descs, items, where = [], [], [], [], [], []
    f32 = False
    for F, vp in jobs:
        frames.append(pack_frame(F))
        f32 = f32 or frames[-1]["f32"]
        blocked.append([1 if (m and m.observations() > 0) else 0 for m in F.mvpMapPoints])
        pos, it = [], []
        for i, p in enumerate(vp):
            if not skipped(p, F):
                pos.append(i), it.append(len(rows))
                r = O.pack_point(p)
                rows.append(r[0]), descs.append(r[1])
                f32 = f32 or r[2]
        items.append(it), where.append(pos)
    return join(frames, blocked, rows, descs, [limit] * len(jobs), list(range(len(jobs))), items, float(th),
                th != 1.0, EPS_F32 if f32 else EPS_F64), where


# ---- the reference's bodies on the objects ----------------------------------------------------------------------------

def frustum_one(F, pMP, limit):
    """Frame.is_in_frustum (Frame.py:328-371), statement by statement on the stand-in objects, so every dtype
    promotion is the reference's."""
    pMP.mbTrackInView = False
    with np.errstate(all="ignore"):
        P = pMP.get_world_pos()
        Pc = F.mRcw @ P + F.mtcw
        PcX = Pc[0]
        PcY = Pc[1]
        PcZ = Pc[2]
        if PcZ < 0.0:
            return False
        invz = 1.0 / PcZ
        u = F.fx * PcX * invz + F.cx
        v = F.fy * PcY * invz + F.cy
        if u < F.mnMinX or u > F.mnMaxX:
            return False
        if v < F.mnMinY or v > F.mnMaxY:
            return False
        max_distance = pMP.get_max_distance_invariance()
        min_distance = pMP.get_min_distance_invariance()
        PO = P - F.mOw
        dist = np.linalg.norm(PO)
        if dist < min_distance or dist > max_distance:
            return False
        Pn = pMP.get_normal()
        view_cos = (PO.T).dot(Pn) / dist
        if view_cos[0] < limit:
            return False
        n_predicted_level = pMP.predict_scale(dist, F)
        pMP.mbTrackInView = True
        pMP.mTrackProjX = u
        pMP.mTrackProjXR = u - F.mbf * invz
        pMP.mTrackProjY = v
        pMP.mnTrackScaleLevel = n_predicted_level
        pMP.mTrackViewCos = view_cos
    return True


def radius_by_viewing_cos(view_cos):
    return 2.5 if view_cos > 0.998 else 4.0


def fp_one(F, pMP, th, nnratio, stats=None):
    """The body of ORBMatcher.search_by_projection_f_p's loop (ORBMatcher.py:226-281) for one point that is tracked
    in view and not bad, against the frame's current slots: True when it assigned.  stats["ratio"] counts the ratio
    test's rejections."""
    b_factor = th != 1.0
    lvl = pMP.mnTrackScaleLevel
    r = radius_by_viewing_cos(pMP.mTrackViewCos)
    if b_factor:
        r *= th
    v_indices = F.get_features_in_area(pMP.mTrackProjX, pMP.mTrackProjY, r * F.mvScaleFactors[lvl], lvl - 1, lvl)
    if not v_indices:
        return False
    d_mp = pMP.get_descriptor()
    best_dist, best_level, best_dist2, best_level2, best_idx = 256, -1, 256, -1, -1
    for idx in v_indices:
        if F.mvpMapPoints[idx]:
            if F.mvpMapPoints[idx].observations() > 0:
                continue
        if F.mvuRight[idx] > 0:
            er = abs(pMP.mTrackProjXR - F.mvuRight[idx])
            if er > r * F.mvScaleFactors[lvl]:
                continue
        dist = O.popcount(d_mp, F.mDescriptors[idx])
        if dist < best_dist:
            best_dist2, best_dist = best_dist, dist
            best_level2, best_level = best_level, F.mvKeysUn[idx].octave
            best_idx = idx
        elif dist < best_dist2:
            best_level2 = F.mvKeysUn[idx].octave
            best_dist2 = dist
    if best_dist <= TH_HIGH:
        if best_level == best_level2 and best_dist > nnratio * best_dist2:
            if stats is not None:
                stats["ratio"] += 1
            return False
        F.mvpMapPoints[best_idx] = pMP
        return True
    return False


def loop(F, vp, th, limit, nnratio):
    """Tracking.search_local_points (Tracking.py:439-468) on the stand-in objects, body by body."""
    n_to_match = 0
    for pMP in vp:
        if pMP.mnLastFrameSeen == F.mnId:
            continue
        if pMP.is_bad():
            continue
        if frustum_one(F, pMP, limit):
            pMP.increase_visible()
            n_to_match += 1
    if n_to_match == 0:
        return 0, None
    n = 0
    for pMP in vp:
        if not pMP.mbTrackInView:
            continue
        if pMP.is_bad():
            continue
        n += int(fp_one(F, pMP, th, nnratio))
    return n_to_match, n


def _taken(F, idx):
    m = F.mvpMapPoints[idx]
    return bool(m) and m.observations() > 0


def replay(jobs, th, limit, nnratio, results=None, stats=None):
    """[search_local_points(F, vp, th, limit) for (F, vp) in jobs] from array results over pack(jobs, th, limit) taken
    BEFORE the first assignment (None: computed here with search; a callable: called with the arrays).  The frustum
    half: an unmarked item's in_view stands, a marked one is decided by frustum_one; the attributes of every point in
    view come from frustum_one.  The search half, in list order: a marked item, an item whose best or second feature
    a point with observations has taken meanwhile, and a skipped point that is still tracked in view are redone by
    fp_one against the current slots; the others stand.  stats counts the items (items), those in view (in_view), the
    marked ones (marginal), those redone because a feature was taken (taken), the stale points searched (stale), the
    ratio test's rejections (ratio) and every fp_one call as its (search, list position) (redone)."""
    a, where = pack(jobs, th, limit)
    if results is None or callable(results):
        results = (results or search)(a)
    res = dict(zip(OUTPUTS, results))
    stats = {} if stats is None else stats
    for key in ("items", "in_view", "marginal", "taken", "stale", "ratio"):
        stats.setdefault(key, 0)
    stats.setdefault("redone", [])
    out = []
    for s, (F, vp) in enumerate(jobs):
        at = {i: int(a["srch_off"][s]) + c for c, i in enumerate(where[s])}
        n_to_match = 0
        view = {}
        for i, j in at.items():
            pMP = vp[i]
            stats["items"] += 1
            stats["marginal"] += int(res["status"][j] != 0)
            if res["status"][j] or res["in_view"][j]:
                seen = frustum_one(F, pMP, limit)
                assert res["status"][j] or seen, ("an unmarked item in view that the reference leaves out", s, i)
            else:
                pMP.mbTrackInView = False
                seen = False
            view[i] = seen
            if seen:
                assert res["status"][j] or pMP.mnTrackScaleLevel == res["level"][j], (s, i)
                pMP.increase_visible()
                n_to_match += 1
        stats["in_view"] += n_to_match
        if n_to_match == 0:
            out.append((0, None))
            continue
        n = 0
        for i, pMP in enumerate(vp):
            j = at.get(i)
            if j is None:
                if pMP.mbTrackInView and not pMP.is_bad():
                    stats["stale"] += 1
                    stats["redone"].append((s, i))
                    n += int(fp_one(F, pMP, th, nnratio, stats))
                continue
            if not view[i]:
                continue
            bi, bd, si, sd = (int(res[k][j]) for k in ("best_idx", "best_dist", "second_idx", "second_dist"))
            if res["status"][j]:
                stats["redone"].append((s, i))
                n += int(fp_one(F, pMP, th, nnratio, stats))
                continue
            if bi < 0 or bd > TH_HIGH:
                continue
            if _taken(F, bi) or (si >= 0 and _taken(F, si)):
                stats["taken"] += 1
                stats["redone"].append((s, i))
                n += int(fp_one(F, pMP, th, nnratio, stats))
                continue
            level2, dist2 = (F.mvKeysUn[si].octave, sd) if si >= 0 and sd < 256 else (-1, 256)
            if F.mvKeysUn[bi].octave == level2 and bd > nnratio * dist2:
                stats["ratio"] += 1
                continue
            F.mvpMapPoints[bi] = pMP
            n += 1
        out.append((n_to_match, n))
    return out
