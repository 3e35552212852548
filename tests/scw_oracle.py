"""NumPy / Python restatement of k_scw_search (include/orbfe.h, orbfe_scw_search) over the entry's own arrays, for the
tests: the search half of ORBMatcher.fuse_kf_scw_mp (ORBMatcher.py:409-468) and of search_by_projection_ckf_scw_mp
(:863-916) in float64 with the error bound and the ORBFE_FUSE_MARGINAL bit of the device, operation for operation.
Phase 1 is fuse_oracle.geometry with the bf slot at zero (k_scw_search does not read it; the right coordinate that
geometry still carries is then u itself and changes no decision below 1e308).  Phase 2 is stated here, because
fuse_oracle.search_item with chi_gate=False still marks an item at the chi-square's threshold and knows no blocked
byte: no chi-square, the blocked byte first.  Also the reference's two loop bodies on the stand-in objects of
tests/matcher_world.py (what a marked item is redone with), the packing of such objects and both ordered replays.
"""
from __future__ import annotations

import numpy as np

import fuse_oracle as O

MARGINAL, KF_F64, PT_F64 = O.MARGINAL, O.KF_F64, O.PT_F64
EPS_F32, EPS_F64, TH_LOW = O.EPS_F32, O.EPS_F64, O.TH_LOW

ARRAYS = ("kf_f64", "kf_i32", "off", "xy", "octave", "desc", "blocked", "cell_at", "cell_off", "idx_at", "cell_idx",
          "lvl_off", "scale", "pt_f64", "pt_desc")


def geometry(K, ki, scale, P, th, eps):
    """Phase 1 for one item: (status, None) when it ends before the candidates, else (status, (u, v, Eu, Ev, r,
    level, x0, x1, y0, y1))."""
    K = [float(x) for x in K]
    K[4] = 0.0
    st, g = O.geometry(K, ki, scale, P, th, eps)
    if g is None:
        return st, None
    u, v, _, Eu, Ev, _, r, level, x0, x1, y0, y1 = g
    return st, (u, v, Eu, Ev, r, level, x0, x1, y0, y1)


def _window(a, k, i):
    lo = int(a["lvl_off"][k])
    ki = a["kf_i32"][k]
    return geometry(a["kf_f64"][k], ki, a["scale"][lo:lo + int(ki[2])], a["pt_f64"][i], float(a["th"]), a["eps"])


def search_item(a, k, i, blocked_mask=True, octave_gate=True, radius_gate=True, early_tie=True):
    """(best_idx, best_dist, status) of keyframe k and point i of the arrays `a` (the entry's arguments by name,
    plus th and eps).  The switches exist for the non-vacuity tests only."""
    eps = a["eps"]
    rows = int(a["kf_i32"][k][1])
    st, g = _window(a, k, i)
    if g is None:
        return -1, -1, st
    u, v, Eu, Ev, r, level, x0, x1, y0, y1 = g
    base = int(a["off"][k])
    coff = a["cell_off"][int(a["cell_at"][k]):]
    cidx = a["cell_idx"][int(a["idx_at"][k]):]
    blk = a.get("blocked")
    er_r = eps * abs(r)
    best = None
    for ix in range(x0, x1 + 1):
        for pos in range(int(coff[ix * rows + y0]), int(coff[ix * rows + y1 + 1])):
            f = int(cidx[pos])
            if blocked_mask and blk is not None and blk[base + f]:
                continue
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
            d = O.popcount(a["desc"][base + f], a["pt_desc"][i])
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
    return _window(a, k, i)[1] is not None


# ---- arrays ------------------------------------------------------------------------------------------------------

def from_fuse(a, blocked=None):
    """The entry's arrays from fuse_oracle.join's (u_right and inv_sigma2 fall away)."""
    b = {k: a[k] for k in ARRAYS if k != "blocked"}
    b["blocked"] = None if blocked is None else np.ascontiguousarray(blocked, np.uint8)
    b["th"], b["eps"] = a["th"], a["eps"]
    return b


def fuse_pose(Scw):
    """ORBMatcher.py:398-402."""
    sRcw = Scw[:3, :3]
    scw = np.sqrt(np.dot(sRcw[0], sRcw[0]))
    Rcw = sRcw / scw
    tcw = Scw[:3, 3:4] / scw
    return Rcw, tcw, -Rcw.T @ tcw


def ckf_pose(Scw):
    """ORBMatcher.py:853-857."""
    sRcw = Scw[:3, :3]
    scw = np.linalg.norm(sRcw[0])
    Rcw = sRcw / scw
    tcw = Scw[:3, 3:4] / scw
    return Rcw, tcw, -Rcw.T @ tcw


def with_pose(frame, pose):
    """A keyframe dict (fuse_oracle.pack_kf) with the pose slots taken from (Rcw, tcw, Ow)."""
    f = dict(frame)
    f["f64"] = np.array(frame["f64"], np.float64)
    f["f64"][5:20] = [float(x) for part in pose for x in np.asarray(part).reshape(-1)]
    return f


def pack(kfs, Scws, points, th, blocked=None, pose=fuse_pose):
    """Arrays of stand-in keyframes with one Scw each and map points (every point is sent, in order)."""
    frames = [with_pose(O.pack_kf(kf), pose(S)) for kf, S in zip(kfs, Scws)]
    pts = [O.pack_point(p) for p in points]
    f32 = any(S.dtype == np.float32 for S in Scws) or any(p[2] for p in pts)
    return from_fuse(O.join(frames, [p[0] for p in pts], [p[1] for p in pts], th, EPS_F32 if f32 else EPS_F64), blocked)


# ---- the reference's loop bodies on the objects ----------------------------------------------------------------------

def single_item(kf, pMP, pose, th, vpMatched=None):
    """(bestDist, bestIdx) of ORBMatcher.py:415-468 (vpMatched None) or :867-916 (against vpMatched) for one point,
    statement by statement on the stand-in objects, so every dtype promotion is the reference's."""
    Rcw, tcw, Ow = pose
    ckf = vpMatched is not None
    none = (256 if ckf else float("inf"), -1)
    with np.errstate(all="ignore"):
        p3Dw = pMP.get_world_pos()
        p3Dc = Rcw @ p3Dw + tcw
        if ckf:
            if p3Dc[2][0] <= 0.0:
                return none
            invz = 1.0 / p3Dc[2]
            x, y = p3Dc[0] * invz, p3Dc[1] * invz
        else:
            if p3Dc[2][0] < 0.0:
                return none
            invz = 1.0 / p3Dc[2][0]
            x, y = p3Dc[0][0] * invz, p3Dc[1][0] * invz
        u, v = kf.fx * x + kf.cx, kf.fy * y + kf.cy
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
        bestDist, bestIdx = none
        for idx in vIndices:
            if ckf and vpMatched[idx] is not None:
                continue
            kpLevel = kf.mvKeysUn[idx].octave
            if kpLevel < nPredictedLevel - 1 or kpLevel > nPredictedLevel:
                continue
            dist = O.popcount(dMP, kf.mDescriptors[idx])
            if dist < bestDist:
                bestDist, bestIdx = dist, idx
    return bestDist, bestIdx


STATS = ("reached", "marginal", "changed", "direct", "already_later", "taken", "replaced", "slot_bad", "added")


def _count(a, st, stats):
    for k in range(st.shape[0]):
        for c in range(st.shape[1]):
            if reaches_candidates(a, k, c):
                stats["reached"] += 1
                stats["marginal"] += int(st[k, c] != 0)


def replay_fuse(kfs, Scws, points, th, after=None, results=None, stats=None):
    """The loop `r = fuse_kf_scw_mp(kf, Scw, points, th, [None] * len(points)); after(kf, r[1])` over the keyframes
    from array results (best_idx, best_dist, status over pack(kfs, Scws, points, th), taken BEFORE the first side
    effect; None: computed here with search; a callable: called with the arrays), with marked items and items whose descriptor has changed since
    resolved by single_item.  Returns [(nFused, vpReplacePoint)].  stats counts: items that reach a window
    (reached), marked ones among them (marginal), redone for a changed descriptor (changed), taken as they came
    (direct), points skipped because a replace after an earlier keyframe of this call put them into the keyframe
    (already_later), and the branches of :470-478 (replaced, slot_bad, added)."""
    a = pack(kfs, Scws, points, th)
    if results is None or callable(results):
        results = (results or search)(a)
    bi, bd, st = results
    snaps = [p.get_descriptor().tobytes() for p in points]
    start = [kf.get_map_points() for kf in kfs]
    stats = {} if stats is None else stats
    for key in STATS:
        stats.setdefault(key, 0)
    _count(a, st, stats)
    out = []
    for k, (kf, Scw) in enumerate(zip(kfs, Scws)):
        pose = fuse_pose(Scw)
        found = kf.get_map_points()
        rep, n = [None] * len(points), 0
        for i, pMP in enumerate(points):
            if pMP.is_bad() or pMP in found:
                stats["already_later"] += int(not pMP.is_bad() and pMP not in start[k])
                continue
            if st[k, i]:
                dist, idx = single_item(kf, pMP, pose, th)
            elif bi[k, i] >= 0 and pMP.get_descriptor().tobytes() != snaps[i]:
                stats["changed"] += 1
                dist, idx = single_item(kf, pMP, pose, th)
            else:
                stats["direct"] += 1
                dist, idx = (int(bd[k, i]), int(bi[k, i])) if bi[k, i] >= 0 else (float("inf"), -1)
            if dist <= TH_LOW:
                inkf = kf.get_map_point(idx)
                if inkf:
                    if not inkf.is_bad():
                        rep[i] = inkf
                        stats["replaced"] += 1
                    else:
                        stats["slot_bad"] += 1
                else:
                    pMP.add_observation(kf, idx)
                    kf.add_map_point(pMP, idx)
                    stats["added"] += 1
                n += 1
        if after is not None:
            after(kf, rep)
        out.append((n, rep))
    return out


def replay_ckf(kf, Scw, points, vpMatched, th, results=None, stats=None):
    """search_by_projection_ckf_scw_mp from array results over pack([kf], [Scw], [the points that pass the
    prefilter], th, blocked, ckf_pose): (nmatches, vpMatched).  A marked item, and one whose candidate an earlier
    point of the call has taken (stats: taken), is resolved by single_item against the current vpMatched."""
    found = set(vpMatched) - {None}
    sent = [i for i, p in enumerate(points) if not (p.is_bad() or p in found)]
    blocked = np.array([m is not None for m in vpMatched], np.uint8)
    a = pack([kf], [Scw], [points[i] for i in sent], th, blocked, ckf_pose)
    if results is None or callable(results):
        results = (results or search)(a)
    bi, bd, st = results
    stats = {} if stats is None else stats
    for key in STATS:
        stats.setdefault(key, 0)
    _count(a, st, stats)
    pose = ckf_pose(Scw)
    n = 0
    for c, i in enumerate(sent):
        pMP = points[i]
        if st[0, c]:
            dist, idx = single_item(kf, pMP, pose, th, vpMatched)
        elif bi[0, c] >= 0 and vpMatched[int(bi[0, c])] is not None:
            stats["taken"] += int(bd[0, c] <= TH_LOW)
            dist, idx = single_item(kf, pMP, pose, th, vpMatched)
        else:
            stats["direct"] += 1
            dist, idx = (int(bd[0, c]), int(bi[0, c])) if bi[0, c] >= 0 else (256, -1)
        if dist <= TH_LOW:
            vpMatched[idx] = pMP
            n += 1
    return n, vpMatched
