"""NumPy / Python restatement of k_fkf_search (include/orbfe.h, orbfe_fkf_search) over the entry's own arrays, for the
tests: the search half of ORBMatcher.search_by_projection_f_kf_f (ORBMatcher.py:936-983, with
Frame.get_features_in_area, Frame.py:373-416) in float64 with the error bound and the ORBFE_FUSE_MARGINAL bit of the
device, operation for operation.  A search is a target frame and a list of rows of one shared point table; a frame
carries one blocked byte per feature.

The switches of `geometry` / `search_item` exist for the non-vacuity tests only; each turns one property of the mode off
and gives what a keyframe search would give:
    depth_gate       pc.z < 0 ends the item
    exclusive_max    u == mnMaxX and v == mnMaxY are outside
    floor_ceil       the cell window is floor .. ceil, not trunc .. trunc
    two_octaves      a candidate's octave lies in [level - 1, level]
    viewing_gate     the viewing-cosine gate is left in
    blocked          False: the blocked bytes are not looked at

Also the reference's loop body on the stand-in objects of tests/fkf_cases.py (what a marked or overtaken item is redone
with), the packing of such objects into the arrays, and the whole search_by_projection_f_kf_f from array results
(`replay`).
"""
from __future__ import annotations

import math

import numpy as np

import fuse_oracle as O
from bow_match_oracle import HISTO_LENGTH, cut_is_stable, three_maxima
from fuse_oracle import _div, _isfinite, _log, _near_int

MARGINAL, KF_F64, PT_F64 = O.MARGINAL, O.KF_F64, O.PT_F64
EPS_F32, EPS_F64 = O.EPS_F32, O.EPS_F64

KF_ARRAYS = ("kf_f64", "kf_i32", "off", "xy", "octave", "desc", "blocked", "cell_at", "cell_off", "idx_at", "cell_idx",
             "lvl_off", "scale")
ARRAYS = KF_ARRAYS + ("pt_f64", "pt_desc", "srch_kf", "srch_off", "item_pt")


def geometry(K, ki, scale, P, th, eps, depth_gate=False, exclusive_max=False, floor_ceil=False, viewing_gate=False):
    """Phase 1 of the kernel for one item: (status, None) when the item ends before the candidates, else
    (status, (u, v, Eu, Ev, r, level, x0, x1, y0, y1))."""
    K, P = [float(x) for x in K], [float(x) for x in P]
    cols, rows, levels = (int(x) for x in ki)
    fx, fy, cx, cy = K[0:4]
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
        return 0, None
    if zc == 0.0 or abs(zc) < Ez:
        return MARGINAL, None
    with np.errstate(all="ignore"):
        iz = _div(1.0, zc)
        aiz = abs(iz)
        xn, yn = float(f(fx) * xc), float(f(fy) * yc)
        fxx, fyy = float(f(xn) * iz), float(f(yn) * iz)
        u, v = float(f(fxx) + cx), float(f(fyy) + cy)
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
        tot = float(((f(u) + v) + Eu) + Ev)
    if not _isfinite(tot):
        return MARGINAL, None
    if (abs(u - minX) < Eu + eps * abs(minX) or abs(u - maxX) < Eu + eps * abs(maxX)
            or abs(v - minY) < Ev + eps * abs(minY) or abs(v - maxY) < Ev + eps * abs(maxY)):
        st = MARGINAL
    if exclusive_max:
        outside = not (minX <= u < maxX and minY <= v < maxY)
    else:
        outside = u < minX or u > maxX or v < minY or v > maxY
    if outside:
        return st, None
    po0, po1, po2 = p0 - K[17], p1 - K[18], p2 - K[19]
    with np.errstate(all="ignore"):
        dist = float(np.sqrt(f((f(po0) * po0 + f(po1) * po1) + f(po2) * po2)))
    Ed = 6.0 * eps * dist
    minD, maxD = P[6], P[7]
    if not _isfinite(dist):
        return MARGINAL, None
    if abs(dist - minD) < Ed + eps * abs(minD) or abs(dist - maxD) < Ed + eps * abs(maxD):
        st = MARGINAL
    if dist < minD or dist > maxD:
        return st, None
    if viewing_gate and not (po0 * P[3] + po1 * P[4]) + po2 * P[5] >= 0.5 * dist:
        return st, None
    q = _div(_log(_div(P[8], dist)), lsf)
    if not _isfinite(q):
        return MARGINAL, None
    if _near_int(q, _div(10.0 * eps, abs(lsf)) + 4.0 * eps * abs(q)):
        st = MARGINAL
    cq = math.ceil(q)
    level = 0 if cq < 0 else (levels - 1 if cq > levels - 1 else int(cq))
    r = th * float(scale[level])
    with np.errstate(all="ignore"):
        ax, bx = float((f(u - minX) - r) * winv), float((f(u - minX) + r) * winv)
        ay, by = float((f(v - minY) - r) * hinv), float((f(v - minY) + r) * hinv)
        tot = float((f(ax) + bx) + (f(ay) + by))
    if not _isfinite(tot):
        return MARGINAL, None
    Ewx = abs(winv) * (Eu + 4.0 * eps * ((abs(u) + abs(minX)) + abs(r)))
    Ewy = abs(hinv) * (Ev + 4.0 * eps * ((abs(v) + abs(minY)) + abs(r)))
    if floor_ceil:
        lo_x, hi_x, lo_y, hi_y = math.floor(ax), math.ceil(bx), math.floor(ay), math.ceil(by)
    else:
        # int() truncates toward zero: (-1, 1) is cell 0, so only an integer of magnitude >= 1 separates two outcomes
        if any(abs(a) > 0.5 and _near_int(a, E) for a, E in ((ax, Ewx), (bx, Ewx), (ay, Ewy), (by, Ewy))):
            st = MARGINAL
        lo_x, hi_x, lo_y, hi_y = math.trunc(ax), math.trunc(bx), math.trunc(ay), math.trunc(by)
    if lo_x >= cols or hi_x < 0 or lo_y >= rows or hi_y < 0:
        return st, None
    x0, x1 = max(0, lo_x), min(cols - 1, hi_x)
    y0, y1 = max(0, lo_y), min(rows - 1, hi_y)
    return st, (u, v, Eu, Ev, r, level, x0, x1, y0, y1)


def search_of(a, i):
    """The search that owns item i."""
    return int(np.searchsorted(np.asarray(a["srch_off"]), i, side="right")) - 1


def _window(a, s, i, **kw):
    k = int(a["srch_kf"][s])
    lo = int(a["lvl_off"][k])
    ki = a["kf_i32"][k]
    row = int(a["item_pt"][i])
    return k, row, geometry(a["kf_f64"][k], ki, a["scale"][lo:lo + int(ki[2])], a["pt_f64"][row], float(a["th"]),
                            a["eps"], **kw)


def search_item(a, s, i, early_tie=True, two_octaves=False, blocked=True, **kw):
    """(best_idx, best_dist, status) of item i, which belongs to search s, of the arrays `a` (the entry's arguments
    by name, plus th and eps)."""
    eps = a["eps"]
    k, row, (st, g) = _window(a, s, i, **kw)
    if g is None:
        return -1, -1, st
    rows = int(a["kf_i32"][k][1])
    u, v, Eu, Ev, r, level, x0, x1, y0, y1 = g
    base = int(a["off"][k])
    coff = a["cell_off"][int(a["cell_at"][k]):]
    cidx = a["cell_idx"][int(a["idx_at"][k]):]
    blk = a["blocked"] if blocked else None
    er_r = eps * abs(r)
    best = None
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
            if o < level - 1 or o > level + (0 if two_octaves else 1):
                continue
            d = O.popcount(a["desc"][base + f], a["pt_desc"][row])
            key = (d, pos if early_tie else -pos)
            if best is None or key < best[0]:
                best = (key, f, d)
    if best is None:
        return -1, -1, st
    return best[1], best[2], st


def search(a, **kw):
    """best_idx, best_dist int32 and status uint8, flat over the items."""
    off = [int(x) for x in a["srch_off"]]
    n = off[-1] if off else 0
    bi, bd, st = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    for s in range(len(off) - 1):
        for i in range(off[s], off[s + 1]):
            bi[i], bd[i], st[i] = search_item(a, s, i, **kw)
    return bi, bd, st


def reaches_candidates(a, s, i):
    """Whether item i gets as far as a cell window (the denominator of the marginal share)."""
    return _window(a, s, i)[2][1] is not None


# ---- arrays --------------------------------------------------------------------------------------------------------

def join(frames, blocked, pt_f64, pt_desc, srch_kf, items, th, eps):
    """The entry's arrays of frame dicts (pack_frame / fuse_cases.KfBuilder.build), one blocked array per frame (or
    None: nothing blocked anywhere), a point table and per search its target and its list of point rows."""
    a = O.join(frames, pt_f64, pt_desc, th, eps)
    b = {k: a[k] for k in KF_ARRAYS + ("pt_f64", "pt_desc", "th", "eps") if k != "blocked"}
    n = int(a["off"][-1]) if len(frames) else 0
    b["blocked"] = None if blocked is None else np.concatenate(
        [np.asarray(x, np.uint8).reshape(-1) for x in blocked] + [np.zeros(0, np.uint8)])
    assert b["blocked"] is None or len(b["blocked"]) == n
    off = np.zeros(len(items) + 1, np.int64)
    np.cumsum([len(it) for it in items], out=off[1:])
    b.update(srch_kf=np.array(srch_kf, np.int32), srch_off=off,
             item_pt=np.array([r for it in items for r in it], np.int32))
    return b


def pack_frame(F):
    """A frame dict of the reference's Frame surface: the grid FRAME_GRID_COLS x FRAME_GRID_ROWS, the pose of mTcw
    and Ow by the reference's expression (ORBMatcher.py:927-929)."""
    n = len(F.mvKeysUn)
    cols, rows, levels = F.FRAME_GRID_COLS, F.FRAME_GRID_ROWS, F.mnScaleLevels
    Rcw, tcw = F.mTcw[:3, :3], F.mTcw[:3, 3:4]
    Ow = -np.dot(Rcw.T, tcw)
    f64 = [F.fx, F.fy, F.cx, F.cy, 0.0] + [float(x) for part in (Rcw, tcw, Ow) for x in part.reshape(-1)] + [
        F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY, F.mfGridElementWidthInv, F.mfGridElementHeightInv, F.mfLogScaleFactor]
    sizes = [len(F.mGrid[ix][iy]) for ix in range(cols) for iy in range(rows)]
    return dict(f64=np.array(f64, np.float64), i32=np.array([cols, rows, levels], np.int32),
                xy=np.array([k.pt for k in F.mvKeysUn], np.float64).reshape(n, 2),
                octave=np.array([k.octave for k in F.mvKeysUn], np.int32), u_right=np.zeros(n),
                desc=np.asarray(F.mDescriptors, np.uint8).reshape(n, 32),
                cell_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                cell_idx=np.array([g for ix in range(cols) for iy in range(rows) for g in F.mGrid[ix][iy]], np.int32),
                scale=np.array(F.mvScaleFactors[:levels], np.float64), inv_sigma2=np.zeros(levels),
                f32=F.mTcw.dtype == np.float32)


def pack_point(p):
    """fuse_oracle.pack_point without the normal, which the search never asks for: NaN in its slots."""
    pos = p.get_world_pos()
    row = [float(x) for x in pos.reshape(-1)] + [float("nan")] * 3 + [
        p.get_min_distance_invariance(), p.get_max_distance_invariance(), p.mfMaxDistance]
    return row, np.asarray(p.get_descriptor(), np.uint8).reshape(32), pos.dtype == np.float32


def pack(jobs, th):
    """Arrays of search_by_projection_f_kf_f(F, kf, found, th, .) for every (F, kf, found) of jobs (distinct
    frames), one search per job, every surviving point sent, and per search the list positions of its items."""
    frames, blocked, rows, descs, items, where = [], [], [], [], [], []
    f32 = False
    for F, kf, found in jobs:
        frames.append(pack_frame(F))
        f32 = f32 or frames[-1]["f32"]
        blocked.append([1 if m else 0 for m in F.mvpMapPoints])
        pos, it = [], []
        for i, p in enumerate(kf.get_map_point_matches()):
            if p and not p.is_bad() and p not in found:
                pos.append(i), it.append(len(rows))
                r = pack_point(p)
                rows.append(r[0]), descs.append(r[1])
                f32 = f32 or r[2]
        items.append(it), where.append(pos)
    return join(frames, blocked, rows, descs, list(range(len(jobs))), items, th, EPS_F32 if f32 else EPS_F64), where


# ---- the reference's loop body on the objects -------------------------------------------------------------------------

def single_item(F, pMP, th, taken=None):
    """(bestDist, bestIdx2) of ORBMatcher.py:939-983 for one point, statement by statement on the stand-in objects,
    so every dtype promotion is the reference's, and raising what the reference raises.  taken: the list whose truth
    values block a feature (default: the frame's current mvpMapPoints)."""
    taken = F.mvpMapPoints if taken is None else taken
    Rcw = F.mTcw[:3, :3]
    tcw = F.mTcw[:3, 3:4]
    none = (256, -1)
    with np.errstate(all="ignore"):
        Ow = -np.dot(Rcw.T, tcw)
        x3Dw = pMP.get_world_pos()
        x3Dc = np.dot(Rcw, x3Dw) + tcw
        xc = x3Dc[0]
        yc = x3Dc[1]
        invzc = 1.0 / x3Dc[2]
        u = F.fx * xc * invzc + F.cx
        v = F.fy * yc * invzc + F.cy
        if u < F.mnMinX or u > F.mnMaxX or v < F.mnMinY or v > F.mnMaxY:
            return none
        PO = x3Dw - Ow
        dist3D = np.linalg.norm(PO)
        maxDistance = pMP.get_max_distance_invariance()
        minDistance = pMP.get_min_distance_invariance()
        if dist3D < minDistance or dist3D > maxDistance:
            return none
        nPredictedLevel = pMP.predict_scale(dist3D, F)
        radius = th * F.mvScaleFactors[nPredictedLevel]
        vIndices2 = F.get_features_in_area(u, v, radius, nPredictedLevel - 1, nPredictedLevel + 1)
    if not vIndices2:
        return none
    dMP = pMP.get_descriptor()
    bestDist, bestIdx2 = 256, -1
    for i2 in vIndices2:
        if taken[i2]:
            continue
        dist = O.popcount(dMP, F.mDescriptors[i2])
        if dist < bestDist:
            bestDist, bestIdx2 = dist, i2
    return bestDist, bestIdx2


def replay(jobs, th, orb_dist, check_orientation=True, results=None, stats=None, agree=False):
    """[search_by_projection_f_kf_f(F, kf, found, th, orb_dist) for (F, kf, found) in jobs] from array results over
    pack(jobs, th) taken BEFORE the first assignment (None: computed here with search; a callable: called with the
    arrays): in list order, a marked item and an item whose best feature an earlier item of the call has taken are
    redone by single_item against the current slots, the others stand.  stats counts the items (items), those that
    reach a window (reached), the marked ones among them (marginal), the items redone because their feature was
    taken (taken), the matches the rotation histogram removed (rotated), the searched points behind the camera
    (behind) and whether every histogram cut was free of ties (stable).  agree: every unmarked item is also checked
    against single_item over the slots as they were before the call."""
    a, where = pack(jobs, th)
    if results is None or callable(results):
        results = (results or search)(a)
    bi, bd, st = results
    stats = {} if stats is None else stats
    for key in ("items", "reached", "marginal", "taken", "rotated", "behind", "redone"):
        stats.setdefault(key, 0)
    stats.setdefault("stable", True)
    out = []
    factor = 1.0 / HISTO_LENGTH
    for s, (F, kf, _) in enumerate(jobs):
        before = list(F.mvpMapPoints)
        vp = kf.get_map_point_matches()
        rot_hist = [[] for _ in range(HISTO_LENGTH)]
        n = 0
        for c, i in enumerate(where[s]):
            j = int(a["srch_off"][s]) + c
            pMP = vp[i]
            stats["items"] += 1
            if reaches_candidates(a, s, j):
                stats["reached"] += 1
                stats["marginal"] += int(st[j] != 0)
                K = a["kf_f64"][s]
                stats["behind"] += int(float(np.dot(K[11:14], a["pt_f64"][int(a["item_pt"][j])][:3]) + K[16]) < 0)
            if agree and not st[j]:
                dist, idx = single_item(F, pMP, th, before)
                assert (idx, dist if idx >= 0 else -1) == (int(bi[j]), int(bd[j])), (s, i)
            if st[j]:
                stats["redone"] += 1
                dist, idx = single_item(F, pMP, th)
            elif bi[j] >= 0 and bd[j] <= orb_dist and F.mvpMapPoints[int(bi[j])]:
                stats["taken"] += 1
                stats["redone"] += 1
                dist, idx = single_item(F, pMP, th)
            else:
                dist, idx = (int(bd[j]), int(bi[j])) if bi[j] >= 0 else (256, -1)
            if dist <= orb_dist:
                F.mvpMapPoints[idx] = pMP
                n += 1
                if check_orientation:
                    rot = kf.mvKeysUn[i].angle - F.mvKeysUn[idx].angle
                    if rot < 0.0:
                        rot += 360.0
                    b = round(rot * factor)
                    if b == HISTO_LENGTH:
                        b = 0
                    assert 0 <= b < HISTO_LENGTH
                    rot_hist[b].append(idx)
        if check_orientation:
            counts = [len(h) for h in rot_hist]
            stats["stable"] = stats["stable"] and cut_is_stable(np.array(counts))
            keep = [int(k) for k in three_maxima(counts)]
            for b in range(HISTO_LENGTH):
                if b not in keep:
                    for idx in rot_hist[b]:
                        F.mvpMapPoints[idx] = None
                        n -= 1
                        stats["rotated"] += 1
        out.append(n)
    return out
