"""NumPy / Python restatement of k_fuse_search (include/orbfe.h, orbfe_fuse_search) over the entry's own arrays, for
the tests: the search half of ORBMatcher.fuse_pkf_mp (ORBMatcher.py:498-567) in float64 with the error bound and the
ORBFE_FUSE_MARGINAL bit of the device, operation for operation (Python floats are IEEE doubles, nothing contracts).
Also single_item, the reference's loop body on the stand-in objects of tests/matcher_world.py with their own dtypes
(what a marginal item is redone with), pack / pack_world, which build the arrays from such objects without the
product's packing code, and replay, the ordered application of the matches (ORBMatcher.py:569-580).
"""
from __future__ import annotations

import math

import numpy as np

MARGINAL = 1
KF_F64, PT_F64 = 27, 9
EPS_F32, EPS_F64 = 2.0 ** -23, 2.0 ** -48
TH_LOW = 50

ARRAYS = ("kf_f64", "kf_i32", "off", "xy", "octave", "u_right", "desc", "cell_at", "cell_off", "idx_at", "cell_idx",
          "lvl_off", "scale", "inv_sigma2", "pt_f64", "pt_desc")


def _near_int(a, e):
    return abs(a - float(np.rint(a))) < e  # strict, as every margin test: a zero bound means an exact value


def _isfinite(x):
    return math.isfinite(x)


def _div(a, b):
    """IEEE a / b for doubles, with the division by zero Python raises on."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _log(a):
    with np.errstate(all="ignore"):
        return float(np.log(np.float64(a)))


def geometry(K, ki, scale, P, th, eps):
    """Phase 1 of the kernel for one item: (status, None) when the item ends before the candidates, else
    (status, (u, v, ur, Eu, Ev, Eur, r, level, x0, x1, y0, y1))."""
    K = [float(x) for x in K]
    P = [float(x) for x in P]
    cols, rows, levels = (int(x) for x in ki)
    fx, fy, cx, cy, bf = K[0:5]
    minX, maxX, minY, maxY, winv, hinv, lsf = K[20:27]
    p0, p1, p2 = P[0:3]
    xc = ((K[5] * p0 + K[6] * p1) + K[7] * p2) + K[14]
    yc = ((K[8] * p0 + K[9] * p1) + K[10] * p2) + K[15]
    zc = ((K[11] * p0 + K[12] * p1) + K[13] * p2) + K[16]
    Ex = 4.0 * eps * (((abs(K[5] * p0) + abs(K[6] * p1)) + abs(K[7] * p2)) + abs(K[14]))
    Ey = 4.0 * eps * (((abs(K[8] * p0) + abs(K[9] * p1)) + abs(K[10] * p2)) + abs(K[15]))
    Ez = 4.0 * eps * (((abs(K[11] * p0) + abs(K[12] * p1)) + abs(K[13] * p2)) + abs(K[16]))
    st = 0
    if zc < 0.0:
        return (MARGINAL if -zc < Ez else 0), None
    with np.errstate(all="ignore"):
        iz = _div(1.0, zc)
        xn, yn = float(np.float64(xc) * iz), float(np.float64(yc) * iz)
        fxx, fyy = float(np.float64(fx) * xn), float(np.float64(fy) * yn)
        u, v = fxx + cx, fyy + cy
        bz = float(np.float64(bf) * iz)
        ur = u - bz
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
        f = np.float64
        Eiz = float(f(iz) * (f(2.0) * rz + 2.0 * eps))
        Ax = float(f(abs(xc)) * Eiz + f(Ex) * (f(iz) + Eiz))
        Ay = float(f(abs(yc)) * Eiz + f(Ey) * (f(iz) + Eiz))
        Exn = float(f(Ax) + f(eps) * (f(abs(xn)) + Ax))
        Eyn = float(f(Ay) + f(eps) * (f(abs(yn)) + Ay))
        Mu, Mv = abs(fxx) + abs(cx), abs(fyy) + abs(cy)
        Eu = float(f(abs(fx)) * Exn + f(4.0 * eps) * Mu)
        Ev = float(f(abs(fy)) * Eyn + f(4.0 * eps) * Mv)
        Eur = float((f(Eu) + f(abs(bf)) * Eiz) + f(4.0 * eps) * (f(abs(bz)) + Mu))
        tot = float(((((f(u) + v) + ur) + Eu) + Ev) + Eur)
    if not _isfinite(tot):
        return MARGINAL, None
    if (abs(u - minX) < Eu + eps * abs(minX) or abs(u - maxX) < Eu + eps * abs(maxX)
            or abs(v - minY) < Ev + eps * abs(minY) or abs(v - maxY) < Ev + eps * abs(maxY)):
        st = MARGINAL
    if not inside:
        return st, None
    po0, po1, po2 = p0 - K[17], p1 - K[18], p2 - K[19]
    with np.errstate(all="ignore"):
        dist = float(np.sqrt(np.float64((po0 * po0 + po1 * po1) + po2 * po2)))
    Ed = 6.0 * eps * dist
    minD, maxD = P[6], P[7]
    if not _isfinite(dist):
        return MARGINAL, None
    if abs(dist - minD) < Ed + eps * abs(minD) or abs(dist - maxD) < Ed + eps * abs(maxD):
        st = MARGINAL
    if dist < minD or dist > maxD:
        return st, None
    t0, t1, t2 = po0 * P[3], po1 * P[4], po2 * P[5]
    dot = (t0 + t1) + t2
    half = 0.5 * dist
    if abs(dot - half) < 5.0 * eps * ((abs(t0) + abs(t1)) + abs(t2)) + Ed:
        st = MARGINAL
    if dot < half:
        return st, None
    q = _div(_log(_div(P[8], dist)), lsf)
    if not _isfinite(q):
        return MARGINAL, None
    if _near_int(q, _div(10.0 * eps, abs(lsf)) + 4.0 * eps * abs(q)):
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
    return st, (u, v, ur, Eu, Ev, Eur, r, level, x0, x1, y0, y1)


def popcount(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def search_item(a, k, i, chi_gate=True, octave_gate=True, radius_gate=True, early_tie=True):
    """(best_idx, best_dist, status) of keyframe k and point i of the arrays `a` (the entry's arguments by name,
    plus th and eps).  The gate switches exist for the non-vacuity tests only."""
    eps, th = a["eps"], float(a["th"])
    lo = int(a["lvl_off"][k])
    ki = a["kf_i32"][k]
    rows = int(ki[1])
    scale = a["scale"][lo:lo + int(ki[2])]
    is2 = a["inv_sigma2"][lo:lo + int(ki[2])]
    st, g = geometry(a["kf_f64"][k], ki, scale, a["pt_f64"][i], th, eps)
    if g is None:
        return -1, -1, st
    u, v, ur, Eu, Ev, Eur, r, level, x0, x1, y0, y1 = g
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
            if radius_gate and not (abs(dx) < r and abs(dy) < r):
                continue
            o = int(a["octave"][base + f])
            if octave_gate and (o < level - 1 or o > level):
                continue
            kr = float(a["u_right"][base + f])
            ex, ey = u - kx, v - ky
            bxy = (2.0 * abs(ex) * Edx + Edx * Edx) + (2.0 * abs(ey) * Edy + Edy * Edy)
            if kr >= 0.0:
                er = ur - kr
                Eer = Eur + 2.0 * eps * (abs(kr) + abs(ur))
                e2 = (ex * ex + ey * ey) + er * er
                B = bxy + (2.0 * abs(er) * Eer + Eer * Eer)
                T = 7.8
            else:
                e2 = ex * ex + ey * ey
                B = bxy
                T = 5.99
            chi = e2 * float(is2[o])
            Echi = abs(float(is2[o])) * B + 6.0 * eps * abs(chi)
            if not abs(chi - T) >= Echi + eps * T:
                st = MARGINAL
            if chi_gate and chi > T:
                continue
            d = popcount(a["desc"][base + f], a["pt_desc"][i])
            key = (d, pos if early_tie else -pos)
            if best is None or key < best[0]:
                best = (key, f, d)
    if best is None:
        return -1, -1, st
    return best[1], best[2], st


def search(a, **kw):
    """best_idx, best_dist (K, P) int32 and status (K, P) uint8 of the arrays."""
    K, P = len(a["kf_f64"]), len(a["pt_f64"])
    bi, bd, st = np.full((K, P), -1, np.int32), np.full((K, P), -1, np.int32), np.zeros((K, P), np.uint8)
    for k in range(K):
        for i in range(P):
            bi[k, i], bd[k, i], st[k, i] = search_item(a, k, i, **kw)
    return bi, bd, st


def reaches_candidates(a, k, i):
    """Whether item (k, i) gets as far as a cell window (the denominator of the marginal share)."""
    lo = int(a["lvl_off"][k])
    ki = a["kf_i32"][k]
    return geometry(a["kf_f64"][k], ki, a["scale"][lo:lo + int(ki[2])], a["pt_f64"][i], float(a["th"]),
                    a["eps"])[1] is not None


# ---- arrays from stand-in objects ---------------------------------------------------------------------------------

def pack_kf(kf):
    n = len(kf.mvKeysUn)
    cols, rows, levels = kf.mnGridCols, kf.mnGridRows, kf.mnScaleLevels
    R, t, O = kf.get_rotation(), kf.get_translation(), kf.get_camera_center()
    f64 = [kf.fx, kf.fy, kf.cx, kf.cy, kf.mbf] + [float(x) for x in R.reshape(-1)] + [float(x) for x in t.reshape(-1)] \
        + [float(x) for x in O.reshape(-1)] + [kf.mnMinX, kf.mnMaxX, kf.mnMinY, kf.mnMaxY, kf.mfGridElementWidthInv,
                                                kf.mfGridElementHeightInv, kf.mfLogScaleFactor]
    sizes = [len(kf.mGrid[ix][iy]) for ix in range(cols) for iy in range(rows)]
    return dict(f64=np.array(f64, np.float64), i32=np.array([cols, rows, levels], np.int32),
                xy=np.array([k.pt for k in kf.mvKeysUn], np.float64).reshape(n, 2),
                octave=np.array([k.octave for k in kf.mvKeysUn], np.int32),
                u_right=np.array([float(x) for x in kf.mvuRight], np.float64),
                desc=np.asarray(kf.mDescriptors, np.uint8).reshape(n, 32),
                cell_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                cell_idx=np.array([g for ix in range(cols) for iy in range(rows) for g in kf.mGrid[ix][iy]], np.int32),
                scale=np.array(kf.mvScaleFactors[:levels], np.float64),
                inv_sigma2=np.array(kf.mvInvLevelSigma2[:levels], np.float64),
                f32=any(x.dtype == np.float32 for x in (R, t, O)))


def pack_point(p):
    pos, nrm = p.get_world_pos(), p.get_normal()
    row = [float(x) for x in pos.reshape(-1)] + [float(x) for x in nrm.reshape(-1)] + [
        p.get_min_distance_invariance(), p.get_max_distance_invariance(), p.mfMaxDistance]
    return row, np.asarray(p.get_descriptor(), np.uint8).reshape(32), pos.dtype == np.float32 or nrm.dtype == np.float32


def join(frames, pt_f64, pt_desc, th, eps):
    """The entry's arrays of keyframe dicts (as pack_kf gives them) and point arrays."""
    def offs(key):
        o = np.zeros(len(frames) + 1, np.int64)
        np.cumsum([len(f[key]) for f in frames], out=o[1:])
        return o

    def cat(key, dt, shape=(-1,)):
        if not frames:
            return np.zeros((0,) + tuple(shape[1:]), dt).reshape(shape)
        return np.ascontiguousarray(np.concatenate([np.asarray(f[key], dt).reshape(shape) for f in frames]))
    return dict(kf_f64=np.array([f["f64"] for f in frames], np.float64).reshape(-1, KF_F64),
                kf_i32=np.array([f["i32"] for f in frames], np.int32).reshape(-1, 3), off=offs("xy"),
                xy=cat("xy", np.float64, (-1, 2)), octave=cat("octave", np.int32), u_right=cat("u_right", np.float64),
                desc=cat("desc", np.uint8, (-1, 32)), cell_at=offs("cell_off"), cell_off=cat("cell_off", np.int32),
                idx_at=offs("cell_idx"), cell_idx=cat("cell_idx", np.int32), lvl_off=offs("scale"),
                scale=cat("scale", np.float64), inv_sigma2=cat("inv_sigma2", np.float64),
                pt_f64=np.array(pt_f64, np.float64).reshape(-1, PT_F64),
                pt_desc=np.array(pt_desc, np.uint8).reshape(-1, 32), th=float(th), eps=float(eps))


def pack(kfs, points, th):
    """Arrays of stand-in keyframes and map points (every point is sent, in order)."""
    frames = [pack_kf(kf) for kf in kfs]
    pts = [pack_point(p) for p in points]
    f32 = any(f["f32"] for f in frames) or any(p[2] for p in pts)
    return join(frames, [p[0] for p in pts], [p[1] for p in pts], th, EPS_F32 if f32 else EPS_F64)


# ---- the reference's loop body on the objects ------------------------------------------------------------------------

def single_item(kf, pMP, th):
    """(bestDist, bestIdx) of ORBMatcher.py:498-567 for one point, statement by statement on the stand-in objects,
    so every dtype promotion is the reference's; (inf, -1) when the point is skipped or has no candidate."""
    fx, fy, cx, cy, bf = kf.fx, kf.fy, kf.cx, kf.cy, kf.mbf
    Rcw, tcw, Ow = kf.get_rotation(), kf.get_translation(), kf.get_camera_center()
    none = (float("inf"), -1)
    with np.errstate(all="ignore"):
        p3Dw = pMP.get_world_pos()
        p3Dc = Rcw @ p3Dw + tcw
        if p3Dc[2][0] < 0.0:
            return none
        invz = 1.0 / p3Dc[2][0]
        x = p3Dc[0][0] * invz
        y = p3Dc[1][0] * invz
        u = fx * x + cx
        v = fy * y + cy
        ur = u - bf * invz
        if not kf.is_in_image(u, v):
            return none
        maxDistance = pMP.get_max_distance_invariance()
        minDistance = pMP.get_min_distance_invariance()
        PO = p3Dw - Ow
        dist3D = np.linalg.norm(PO)
        if dist3D < minDistance or dist3D > maxDistance:
            return none
        Pn = pMP.get_normal()
        if np.dot(PO.T, Pn) < 0.5 * dist3D:
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
            kpLevel = kp.octave
            if kpLevel < nPredictedLevel - 1 or kpLevel > nPredictedLevel:
                continue
            if kf.mvuRight[idx] >= 0:
                kpx, kpy, kpr = kp.pt[0], kp.pt[1], kf.mvuRight[idx]
                ex, ey, er = u - kpx, v - kpy, ur - kpr
                e2 = ex ** 2 + ey ** 2 + er ** 2
                if e2 * kf.mvInvLevelSigma2[kpLevel] > 7.8:
                    continue
            else:
                kpx, kpy = kp.pt[0], kp.pt[1]
                ex, ey = u - kpx, v - kpy
                e2 = ex ** 2 + ey ** 2
                if e2 * kf.mvInvLevelSigma2[kpLevel] > 5.99:
                    continue
            dist = popcount(dMP, kf.mDescriptors[idx])
            if dist < bestDist:
                bestDist, bestIdx = dist, idx
    return bestDist, bestIdx


def apply_match(kf, pMP, bestIdx):
    """ORBMatcher.py:570-579; returns which branch ran: "list_replaced" (pMP.replace(pMPinKF)), "slot_replaced"
    (pMPinKF.replace(pMP)), "slot_bad" or "added"."""
    pMPinKF = kf.get_map_point(bestIdx)
    if pMPinKF:
        if not pMPinKF.is_bad():
            if pMPinKF.observations() > pMP.observations():
                pMP.replace(pMPinKF)
                return "list_replaced"
            pMPinKF.replace(pMP)
            return "slot_replaced"
        return "slot_bad"
    pMP.add_observation(kf, bestIdx)
    kf.add_map_point(pMP, bestIdx)
    return "added"


def replay(kfs, points, th, results=None, stats=None):
    """[fuse_pkf_mp(kf, points, th) for kf in kfs] from array results (best_idx, best_dist, status over pack(kfs,
    [the points that are not None], th), taken BEFORE the first side effect; None: computed here with search) with
    marginal items and items whose descriptor has changed since resolved by single_item.  stats counts what
    happened: items that reach the window (reached), marginal ones among them (marginal), redone for a changed
    descriptor (changed), taken as they came (direct), points skipped because an earlier replace of this call made
    them bad (became_bad), and apply_match's branches."""
    sent = [i for i, p in enumerate(points) if p is not None]
    col = {i: c for c, i in enumerate(sent)}
    a = pack(kfs, [points[i] for i in sent], th)
    if results is None:
        results = search(a)
    bi, bd, st = results
    snaps = {i: points[i].get_descriptor().tobytes() for i in sent}
    bad0 = {i for i in sent if points[i].is_bad()}
    stats = {} if stats is None else stats
    for key in ("reached", "marginal", "marginal_all", "changed", "direct", "became_bad", "list_replaced",
                "slot_replaced", "slot_bad", "added"):
        stats.setdefault(key, 0)
    stats["marginal_all"] += int(np.count_nonzero(st))
    for k in range(len(kfs)):
        for c in range(len(sent)):
            if reaches_candidates(a, k, c):
                stats["reached"] += 1
                stats["marginal"] += int(st[k, c] != 0)
    out = []
    for k, kf in enumerate(kfs):
        n = 0
        for i, pMP in enumerate(points):
            if not pMP:
                continue
            if pMP.is_bad() or pMP.is_in_key_frame(kf):
                stats["became_bad"] += int(pMP.is_bad() and i not in bad0)
                continue
            c = col[i]
            if st[k, c]:
                dist, idx = single_item(kf, pMP, th)
            elif bi[k, c] >= 0 and pMP.get_descriptor().tobytes() != snaps[i]:
                stats["changed"] += 1
                dist, idx = single_item(kf, pMP, th)
            else:
                stats["direct"] += 1
                dist, idx = (int(bd[k, c]), int(bi[k, c])) if bi[k, c] >= 0 else (float("inf"), -1)
            if dist <= TH_LOW:
                stats[apply_match(kf, pMP, idx)] += 1
                n += 1
        out.append(n)
    return out
