"""NumPy / Python restatement of k_sim3_search (include/orbfe.h, orbfe_sim3_search) over the entry's own arrays, for
the tests: the search half of both directions of ORBMatcher.search_by_sim3 (ORBMatcher.py:742-789 and :791-838) in
float64 with the error bound and the ORBFE_FUSE_MARGINAL bit of the device, operation for operation.  A search is a
target keyframe, 28 scalars (fx fy cx cy, Rw, tw, sR, t) and a list of rows of one shared point table.

The switches of `geometry` / `search_item` exist for the non-vacuity tests only; each turns one property of the mode
off and gives what a kernel without it would give:
    one_stage = 1 or 2     the camera coordinates are one stage alone (1: Rw p + tw, 2: sR p + t), as k_scw_search's
    target_intrinsics      fx, fy, cx, cy from the target keyframe's block, not from the search
    world_distance         |p - Ow| of the target's block is gated and predicts the level, not |c|
    viewing_gate           the viewing-cosine gate of the other two searches is left in
    identity_items         item i reads row i of the point table, not row item_pt[i]

Also the reference's loop body on the stand-in objects of tests/matcher_world.py (what a marked item is redone with),
the packing of such objects into the arrays, and the whole search_by_sim3 from array results (`replay`).
"""
from __future__ import annotations

import math

import numpy as np

import fuse_oracle as O
from fuse_oracle import _div, _isfinite, _log, _near_int

MARGINAL, KF_F64, PT_F64, SIM3_F64 = O.MARGINAL, O.KF_F64, O.PT_F64, 28
EPS_F32, EPS_F64, TH_HIGH = O.EPS_F32, O.EPS_F64, 100

KF_ARRAYS = ("kf_f64", "kf_i32", "off", "xy", "octave", "desc", "cell_at", "cell_off", "idx_at", "cell_idx", "lvl_off",
             "scale")
ARRAYS = KF_ARRAYS + ("pt_f64", "pt_desc", "srch_f64", "srch_kf", "srch_off", "item_pt")


def _stage(R, t, p, eps):
    """R p + t row by row, sums of three from the left, and 4 eps times the sum of the terms' magnitudes."""
    c, E = [], []
    with np.errstate(all="ignore"):
        for i in range(3):
            a, b, d = float(np.float64(R[3 * i]) * p[0]), float(np.float64(R[3 * i + 1]) * p[1]), float(
                np.float64(R[3 * i + 2]) * p[2])
            c.append(float(((np.float64(a) + b) + d) + t[i]))
            E.append(float(4.0 * eps * (((np.float64(abs(a)) + abs(b)) + abs(d)) + abs(t[i]))))
    return c, E


def geometry(S, K, ki, scale, P, th, eps, one_stage=None, target_intrinsics=False, world_distance=False,
             viewing_gate=False):
    """Phase 1 of the kernel for one item: (status, None) when the item ends before the candidates, else
    (status, (u, v, Eu, Ev, r, level, x0, x1, y0, y1))."""
    S, K, P = [float(x) for x in S], [float(x) for x in K], [float(x) for x in P]
    cols, rows, levels = (int(x) for x in ki)
    fx, fy, cx, cy = K[0:4] if target_intrinsics else S[0:4]
    minX, maxX, minY, maxY, winv, hinv, lsf = K[20:27]
    Rw, tw, sR, t = S[4:13], S[13:16], S[16:25], S[25:28]
    p = P[0:3]
    f = np.float64
    with np.errstate(all="ignore"):
        if one_stage == 1:
            (xc, yc, zc), (Ex, Ey, Ez) = _stage(Rw, tw, p, eps)
        elif one_stage == 2:
            (xc, yc, zc), (Ex, Ey, Ez) = _stage(sR, t, p, eps)
        else:
            c1, E1 = _stage(Rw, tw, p, eps)
            (xc, yc, zc), E2 = _stage(sR, t, c1, eps)
            Ex, Ey, Ez = (float(((f(abs(sR[3 * i])) * E1[0] + f(abs(sR[3 * i + 1])) * E1[1]) + f(abs(sR[3 * i + 2])) * E1[2])
                                + E2[i]) for i in range(3))
        tot = float(((f(xc) + yc) + zc) + ((f(Ex) + Ey) + Ez))
    if not _isfinite(tot):
        return MARGINAL, None
    st = 0
    if zc < 0.0:
        return (MARGINAL if -zc < Ez else 0), None
    with np.errstate(all="ignore"):
        iz = _div(1.0, zc)
        xn, yn = float(f(xc) * iz), float(f(yc) * iz)
        fxx, fyy = float(f(fx) * xn), float(f(fy) * yn)
        u, v = fxx + cx, fyy + cy
    inside = minX <= u < maxX and minY <= v < maxY
    if zc < Ez:
        st = MARGINAL
    if zc == 0.0:
        assert not inside
        return st, None
    rz = Ez / zc
    if not rz <= 0.25:
        st = MARGINAL
    with np.errstate(all="ignore"):
        Eiz = float(f(iz) * (f(2.0) * rz + 2.0 * eps))
        Ax = float(f(abs(xc)) * Eiz + f(Ex) * (f(iz) + Eiz))
        Ay = float(f(abs(yc)) * Eiz + f(Ey) * (f(iz) + Eiz))
        Exn = float(f(Ax) + f(eps) * (f(abs(xn)) + Ax))
        Eyn = float(f(Ay) + f(eps) * (f(abs(yn)) + Ay))
        Mu, Mv = abs(fxx) + abs(cx), abs(fyy) + abs(cy)
        Eu = float(f(abs(fx)) * Exn + f(4.0 * eps) * Mu)
        Ev = float(f(abs(fy)) * Eyn + f(4.0 * eps) * Mv)
        tot = float(((f(u) + v) + Eu) + Ev)
    if not _isfinite(tot):
        return MARGINAL, None
    if (abs(u - minX) < Eu + eps * abs(minX) or abs(u - maxX) < Eu + eps * abs(maxX)
            or abs(v - minY) < Ev + eps * abs(minY) or abs(v - maxY) < Ev + eps * abs(maxY)):
        st = MARGINAL
    if not inside:
        return st, None
    po = [p[0] - K[17], p[1] - K[18], p[2] - K[19]]
    with np.errstate(all="ignore"):
        if world_distance:
            dist = float(np.sqrt(f((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2])))
            Ed = 6.0 * eps * dist
        else:
            dist = float(np.sqrt(f((f(xc) * xc + f(yc) * yc) + f(zc) * zc)))
            Ed = float(((f(Ex) + Ey) + Ez) + 6.0 * eps * f(dist))
    minD, maxD = P[6], P[7]
    if not _isfinite(dist):
        return MARGINAL, None
    if abs(dist - minD) < Ed + eps * abs(minD) or abs(dist - maxD) < Ed + eps * abs(maxD):
        st = MARGINAL
    if dist < minD or dist > maxD:
        return st, None
    if viewing_gate and (po[0] * P[3] + po[1] * P[4]) + po[2] * P[5] < 0.5 * dist:
        return st, None
    q = _div(_log(_div(P[8], dist)), lsf)
    if not _isfinite(q):
        return MARGINAL, None
    rd = _div(Ed, dist)
    if not rd <= 0.25:
        st = MARGINAL
    if _near_int(q, _div(1.5 * rd + 4.0 * eps, abs(lsf)) + 4.0 * eps * abs(q)):
        st = MARGINAL
    cq = math.ceil(q)
    level = 0 if cq < 0 else (levels - 1 if cq > levels - 1 else int(cq))
    r = th * float(scale[level])
    ax, bx = ((u - minX) - r) * winv, ((u - minX) + r) * winv
    ay, by = ((v - minY) - r) * hinv, ((v - minY) + r) * hinv
    if not _isfinite((ax + bx) + (ay + by)):
        return MARGINAL, None
    Ewx = abs(winv) * (Eu + 4.0 * eps * ((abs(u) + abs(minX)) + abs(r)))
    Ewy = abs(hinv) * (Ev + 4.0 * eps * ((abs(v) + abs(minY)) + abs(r)))
    if _near_int(ax, Ewx) or _near_int(bx, Ewx) or _near_int(ay, Ewy) or _near_int(by, Ewy):
        st = MARGINAL
    fax, cbx, fay, cby = math.floor(ax), math.ceil(bx), math.floor(ay), math.ceil(by)
    if fax >= cols or cbx < 0 or fay >= rows or cby < 0:
        return st, None
    x0, x1 = max(0, fax), min(cols - 1, cbx)
    y0, y1 = max(0, fay), min(rows - 1, cby)
    return st, (u, v, Eu, Ev, r, level, x0, x1, y0, y1)


def search_of(a, i):
    """The search that owns item i."""
    return int(np.searchsorted(np.asarray(a["srch_off"]), i, side="right")) - 1


def _window(a, s, i, identity_items=False, **kw):
    k = int(a["srch_kf"][s])
    lo = int(a["lvl_off"][k])
    ki = a["kf_i32"][k]
    row = i % len(a["pt_f64"]) if identity_items else int(a["item_pt"][i])
    return k, row, geometry(a["srch_f64"][s], a["kf_f64"][k], ki, a["scale"][lo:lo + int(ki[2])], a["pt_f64"][row],
                            float(a["th"]), a["eps"], **kw)


def search_item(a, s, i, early_tie=True, **kw):
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
    er_r = eps * abs(r)
    best = None
    for ix in range(x0, x1 + 1):
        for pos in range(int(coff[ix * rows + y0]), int(coff[ix * rows + y1 + 1])):
            f = int(cidx[pos])
            kx, ky = float(a["xy"][base + f][0]), float(a["xy"][base + f][1])
            dx, dy = kx - u, ky - v
            Edx = Eu + 2.0 * eps * (abs(kx) + abs(u))
            Edy = Ev + 2.0 * eps * (abs(ky) + abs(v))
            if abs(abs(dx) - r) < Edx + er_r or abs(abs(dy) - r) < Edy + er_r:
                st = MARGINAL
            if not (abs(dx) < r and abs(dy) < r):
                continue
            o = int(a["octave"][base + f])
            if o < level - 1 or o > level:
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

def srch_row(K, Rw, tw, sR, t):
    return [float(x) for x in K] + [float(x) for part in (Rw, tw, sR, t) for x in np.asarray(part).reshape(-1)]


def join(frames, pt_f64, pt_desc, srch_f64, srch_kf, items, th, eps):
    """The entry's arrays of keyframe dicts (fuse_oracle.pack_kf / fuse_cases.KfBuilder.build), a point table and
    per search its scalars, its target and its list of point rows."""
    a = O.join(frames, pt_f64, pt_desc, th, eps)
    b = {k: a[k] for k in KF_ARRAYS + ("pt_f64", "pt_desc", "th", "eps")}
    off = np.zeros(len(items) + 1, np.int64)
    np.cumsum([len(it) for it in items], out=off[1:])
    b.update(srch_f64=np.array(srch_f64, np.float64).reshape(-1, SIM3_F64), srch_kf=np.array(srch_kf, np.int32),
             srch_off=off, item_pt=np.array([r for it in items for r in it], np.int32))
    return b


def sim3_parts(s12, R12, t12):
    """ORBMatcher.py:720-722."""
    sR12 = s12 * R12
    sR21 = (1.0 / s12) * R12.T
    t21 = -sR21 @ t12
    return sR12, sR21, t21


def already(kf1, kf2, vpMatches12):
    """ORBMatcher.py:729-737."""
    N1, N2 = len(kf1.get_map_point_matches()), len(kf2.get_map_point_matches())
    a1, a2 = [False] * N1, [False] * N2
    for i, pMP in enumerate(vpMatches12):
        if pMP:
            a1[i] = True
            idx2 = pMP.get_index_in_keyframe(kf2)
            if 0 <= idx2 < N2:
                a2[idx2] = True
    return a1, a2


def pack(kf1, pairs, th):
    """Arrays of search_by_sim3(kf1, kf2, vpMatches12, s12, R12, t12, th) for every (kf2, vpMatches12, s12, R12, t12)
    of pairs, two searches per pair, every surviving point sent, and per search the list positions of its items.
    kf1 is keyframe 0 and its live points are the first rows of the point table."""
    kfs, at = [kf1], {id(kf1): 0}
    vp1 = kf1.get_map_point_matches()
    K = (kf1.fx, kf1.fy, kf1.cx, kf1.cy)
    rows, descs, f32 = [], [], False
    row1 = {}
    for i, p in enumerate(vp1):
        if p and not p.is_bad():
            row1[i] = len(rows)
            r = O.pack_point(p)
            rows.append(r[0]), descs.append(r[1])
            f32 = f32 or r[2]
    srch_f64, srch_kf, items, where = [], [], [], []
    for kf2, vm, s12, R12, t12 in pairs:
        if id(kf2) not in at:
            at[id(kf2)] = len(kfs)
            kfs.append(kf2)
        sR12, sR21, t21 = sim3_parts(s12, R12, t12)
        f32 = f32 or any(np.asarray(x).dtype == np.float32 for x in (sR12, sR21, t21, t12))
        a1, a2 = already(kf1, kf2, vm)
        pos1 = [i for i in sorted(row1) if not a1[i]]
        srch_f64.append(srch_row(K, kf1.get_rotation(), kf1.get_translation(), sR21, t21))
        srch_kf.append(at[id(kf2)])
        items.append([row1[i] for i in pos1])
        pos2, it2 = [], []
        for i, p in enumerate(kf2.get_map_point_matches()):
            if not p or a2[i] or p.is_bad():
                continue
            pos2.append(i), it2.append(len(rows))
            r = O.pack_point(p)
            rows.append(r[0]), descs.append(r[1])
            f32 = f32 or r[2]
        srch_f64.append(srch_row(K, kf2.get_rotation(), kf2.get_translation(), sR12, t12))
        srch_kf.append(0)
        items.append(it2)
        where += [pos1, pos2]
    frames = [O.pack_kf(kf) for kf in kfs]
    f32 = f32 or any(fr["f32"] for fr in frames)
    return join(frames, rows, descs, srch_f64, srch_kf, items, th, EPS_F32 if f32 else EPS_F64), where


# ---- the reference's loop body on the objects -------------------------------------------------------------------------

def single_item(pMP, Rw, tw, sR, t, kf, th, K):
    """(bestDist, bestIdx) of ORBMatcher.py:746-786 / :795-835 for one point looked for in kf, statement by
    statement on the stand-in objects, so every dtype promotion is the reference's."""
    fx, fy, cx, cy = K
    none = (float("inf"), -1)
    with np.errstate(all="ignore"):
        p3Dw = pMP.get_world_pos()
        p3Dc1 = Rw @ p3Dw + tw
        p3Dc2 = sR @ p3Dc1 + t
        if p3Dc2[2] < 0.0:
            return none
        invz = 1.0 / p3Dc2[2]
        x, y = p3Dc2[0] * invz, p3Dc2[1] * invz
        u, v = fx * x + cx, fy * y + cy
        if not kf.is_in_image(u, v):
            return none
        maxDistance = pMP.get_max_distance_invariance()
        minDistance = pMP.get_min_distance_invariance()
        dist3D = np.linalg.norm(p3Dc2)
        if not (minDistance <= dist3D <= maxDistance):
            return none
        nPredictedLevel = pMP.predict_scale(dist3D, kf)
        radius = th * kf.mvScaleFactors[nPredictedLevel]
        vIndices = kf.get_features_in_area(u, v, radius)
        if not vIndices:
            return none
        dMP = pMP.get_descriptor()
        bestDist, bestIdx = float("inf"), -1
        for idx in vIndices:
            kp = kf.mvKeysUn[idx]
            if not (nPredictedLevel - 1 <= kp.octave <= nPredictedLevel):
                continue
            dist = O.popcount(dMP, kf.mDescriptors[idx])
            if dist < bestDist:
                bestDist, bestIdx = dist, idx
    return bestDist, bestIdx


def poses(kf1, kf2, s12, R12, t12):
    """Per direction (Rw, tw, sR, t, target keyframe)."""
    sR12, sR21, t21 = sim3_parts(s12, R12, t12)
    return ((kf1.get_rotation(), kf1.get_translation(), sR21, t21, kf2),
            (kf2.get_rotation(), kf2.get_translation(), sR12, t12, kf1))


def replay(kf1, pairs, th, results=None, stats=None, agree=False):
    """[search_by_sim3(kf1, *pair, th) for pair in pairs] from array results over pack(kf1, pairs, th) (None:
    computed here with search; a callable: called with the arrays), marked items redone by single_item.  stats
    counts the items that reach a window (reached), the marked ones among them (marginal) and the direction-1 winners
    the mutual check refuses (refused).  agree: every
    unmarked item is also checked against single_item."""
    a, where = pack(kf1, pairs, th)
    if results is None or callable(results):
        results = (results or search)(a)
    bi, bd, st = results
    stats = {} if stats is None else stats
    for key in ("reached", "marginal", "items", "refused"):
        stats.setdefault(key, 0)
    K = (kf1.fx, kf1.fy, kf1.cx, kf1.cy)
    out = []
    for m, (kf2, vm, s12, R12, t12) in enumerate(pairs):
        vps = (kf1.get_map_point_matches(), kf2.get_map_point_matches())
        match = []
        for d, (Rw, tw, sR, t, target) in enumerate(poses(kf1, kf2, s12, R12, t12)):
            s = 2 * m + d
            best = [-1] * len(vps[d])
            for c, i in enumerate(where[s]):
                j = int(a["srch_off"][s]) + c
                stats["items"] += 1
                if reaches_candidates(a, s, j):
                    stats["reached"] += 1
                    stats["marginal"] += int(st[j] != 0)
                if st[j] or agree:
                    dist, idx = single_item(vps[d][i], Rw, tw, sR, t, target, th, K)
                    if not st[j]:
                        assert (idx, dist if idx >= 0 else -1) == (int(bi[j]), int(bd[j])), (s, i)
                else:
                    dist, idx = (int(bd[j]), int(bi[j])) if bi[j] >= 0 else (float("inf"), -1)
                if dist <= TH_HIGH:
                    best[i] = idx
            match.append(best)
        n = 0
        for i1, idx2 in enumerate(match[0]):
            if idx2 >= 0 and match[1][idx2] == i1:
                vm[i1] = vps[1][idx2]
                n += 1
            elif idx2 >= 0:
                stats["refused"] += 1
        out.append((n, vm))
    return out
