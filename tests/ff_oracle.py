"""NumPy / Python restatement of k_ff_search (include/orbfe.h, orbfe_ff_search) over the entry's own arrays, for the
tests: the search half of ORBMatcher.search_by_projection_f_f (ORBMatcher.py:291-393, with
Frame.get_features_in_area, Frame.py:373-416) in float64 with the error bounds and the ORBFE_FUSE_MARGINAL bit of the
device, operation for operation.  A search is a (current frame, last frame) pair: a target frame, a th, an octave mode
and a list of (row of the shared point table, level); a frame carries one blocked byte and one right coordinate per
feature.

The switches of `search_item` exist for the non-vacuity tests only; each turns one property of the mode off:
    depth_gate       False: pc.z < 0 goes on, as in k_fkf_search
    stereo_gate      False: u_right is not looked at
    fkf_order        the projection multiplies fx * (xc * invz), the keyframe family's order
    blocked          False: the blocked bytes are not looked at
    mode             an octave mode that overrides every search's

Also the reference's body on stand-in objects (what a marked or overtaken item is redone with), the reference's whole
function statement by statement (`loop`), the packing of such objects into the arrays, and the whole
search_by_projection_f_f from array results (`replay`).
"""
from __future__ import annotations

import math

import numpy as np

import fkf_oracle as FK
import fuse_oracle as O
import local_search_oracle as LO
from bow_match_oracle import HISTO_LENGTH, three_maxima
from fuse_oracle import _div, _isfinite, _near_int

MARGINAL, KF_F64, PT_F64 = O.MARGINAL, O.KF_F64, O.PT_F64
EPS_F32, EPS_F64 = O.EPS_F32, O.EPS_F64
TH_HIGH = 100

KF_ARRAYS = LO.KF_ARRAYS
ARRAYS = KF_ARRAYS + ("pt_f64", "pt_desc", "srch_th", "srch_mode", "srch_kf", "srch_off", "item_pt", "item_level")
OUTPUTS = ("best_idx", "best_dist", "status")


def geometry(K, ki, scale, P, level, th, eps, depth_gate=True, fkf_order=True):
    """Phase 1 of the kernel for one item: (status, window).  window is None when the item does not reach the
    candidates, else (u, v, ur, Eu, Ev, Eur, r, x0, x1, y0, y1)."""
    K, P = [float(x) for x in K], [float(x) for x in P]
    cols, rows, _ = (int(x) for x in ki)
    fx, fy, cx, cy, bf = K[0:5]
    minX, maxX, minY, maxY, winv, hinv = K[20:26]
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
        return (MARGINAL if -zc < Ez else 0), None
    if zc < Ez:
        st = MARGINAL
    if zc == 0.0:
        return MARGINAL, None
    with np.errstate(all="ignore"):
        iz = _div(1.0, zc)
        aiz = abs(iz)
        if fkf_order:
            xn, yn = float(f(fx) * xc), float(f(fy) * yc)
            fxx, fyy = float(f(xn) * iz), float(f(yn) * iz)
        else:
            xn, yn = float(f(xc) * iz), float(f(yc) * iz)
            fxx, fyy = float(f(fx) * xn), float(f(fy) * yn)
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
        return MARGINAL, None
    if (abs(u - minX) < Eu + eps * abs(minX) or abs(u - maxX) < Eu + eps * abs(maxX)
            or abs(v - minY) < Ev + eps * abs(minY) or abs(v - maxY) < Ev + eps * abs(maxY)):
        st = MARGINAL
    if u < minX or u > maxX or v < minY or v > maxY:
        return st, None
    with np.errstate(all="ignore"):
        r = float(f(th) * float(scale[level]))
        ax, bx = float((f(u - minX) - r) * winv), float((f(u - minX) + r) * winv)
        ay, by = float((f(v - minY) - r) * hinv), float((f(v - minY) + r) * hinv)
        tot = float((f(ax) + bx) + (f(ay) + by))
    if not _isfinite(tot):
        return MARGINAL, None
    Ewx = abs(winv) * (Eu + 4.0 * eps * ((abs(u) + abs(minX)) + abs(r)))
    Ewy = abs(hinv) * (Ev + 4.0 * eps * ((abs(v) + abs(minY)) + abs(r)))
    # int() truncates toward zero: (-1, 1) is cell 0, so only an integer of magnitude >= 1 separates two outcomes
    if any(abs(a) > 0.5 and _near_int(a, E) for a, E in ((ax, Ewx), (bx, Ewx), (ay, Ewy), (by, Ewy))):
        st = MARGINAL
    lo_x, hi_x, lo_y, hi_y = math.trunc(ax), math.trunc(bx), math.trunc(ay), math.trunc(by)
    if lo_x >= cols or hi_x < 0 or lo_y >= rows or hi_y < 0:
        return st, None
    x0, x1 = max(0, lo_x), min(cols - 1, hi_x)
    y0, y1 = max(0, lo_y), min(rows - 1, hi_y)
    return st, (u, v, ur, Eu, Ev, Eur, r, x0, x1, y0, y1)


search_of = FK.search_of


def octave_range(mode, level):
    """[lo, hi] of a candidate's octave: what the three get_features_in_area calls of ORBMatcher.py:334-341 keep."""
    if mode == 1:
        return level, 2 ** 31 - 1
    if mode == 2:
        return 0, level
    return level - 1, level + 1


def _window(a, s, i, **kw):
    k = int(a["srch_kf"][s])
    lo = int(a["lvl_off"][k])
    ki = a["kf_i32"][k]
    row = int(a["item_pt"][i])
    return k, row, geometry(a["kf_f64"][k], ki, a["scale"][lo:lo + int(ki[2])], a["pt_f64"][row],
                            int(a["item_level"][i]), float(a["srch_th"][s]), a["eps"], **kw)


def candidates(a, s, i, stereo_gate=True, blocked=True, mode=None, **kw):
    """(status, [(distance, position, feature)] in visiting order) of item i of search s."""
    eps = a["eps"]
    k, row, (st, g) = _window(a, s, i, **kw)
    if g is None:
        return st, []
    rows = int(a["kf_i32"][k][1])
    u, v, ur, Eu, Ev, Eur, r, x0, x1, y0, y1 = g
    olo, ohi = octave_range(int(a["srch_mode"][s]) if mode is None else mode, int(a["item_level"][i]))
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
            if o < olo or o > ohi:
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
    return st, out


def search_item(a, s, i, **kw):
    """(best_idx, best_dist, status) of item i, which belongs to search s, of the arrays `a` (the entry's arguments by
    name, plus eps): the smallest key (distance, visiting position)."""
    st, cand = candidates(a, s, i, **kw)
    if not cand:
        return -1, -1, st
    d, _, f = min(cand)
    return f, d, st


def search(a, **kw):
    """best_idx, best_dist int32 and status uint8, flat over the items."""
    off = [int(x) for x in a["srch_off"]]
    n = off[-1] if off else 0
    bi, bd, st = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    for s in range(len(off) - 1):
        for i in range(off[s], off[s + 1]):
            bi[i], bd[i], st[i] = search_item(a, s, i, **kw)
    return bi, bd, st


# ---- arrays --------------------------------------------------------------------------------------------------------

def join(frames, blocked, pt_f64, pt_desc, ths, modes, srch_kf, items, levels, eps):
    """The entry's arrays of frame dicts (pack_frame / fuse_cases.KfBuilder.build), one blocked array per frame (or
    None: nothing blocked anywhere), a point table and per search its th, its mode, its target, its list of point rows
    and their levels."""
    b = LO.join(frames, blocked, pt_f64, pt_desc, [0.0] * len(srch_kf), srch_kf, items, 0.0, False, eps)
    for k in ("srch_limit", "th", "th_on"):
        del b[k]
    b["srch_th"] = np.array(ths, np.float64).reshape(-1)
    b["srch_mode"] = np.array(modes, np.int32).reshape(-1)
    b["item_level"] = np.array([x for lv in levels for x in lv], np.int32)
    assert len(b["item_level"]) == len(b["item_pt"])
    return b


def pack_frame(F):
    """A frame dict of the reference's Frame surface (the pose from mTcw, bf, the right coordinates)."""
    return LO.pack_frame(F)


def mode_of(cur, last):
    """1 where the reference's b_forward holds, else 2 where its b_backward holds, else 0 (ORBMatcher.py:297-308)."""
    Rcw = cur.mTcw[:3, :3]
    tcw = cur.mTcw[:3, 3:4]
    twc = -Rcw.T @ tcw
    Rlw = last.mTcw[:3, :3]
    tlw = last.mTcw[:3, 3:4]
    tlc = Rlw @ twc + tlw
    b_forward = tlc[2] > cur.mb
    b_backward = -tlc[2] > cur.mb
    return 1 if b_forward else (2 if b_backward else 0)


def expressible(p):
    pos = p.get_world_pos()
    return (type(pos) is np.ndarray and pos.shape == (3, 1) and pos.dtype in (np.float32, np.float64)
            and bool(np.isfinite(pos).all()))


def pack(jobs):
    """Arrays of search_by_projection_f_f(cur, last, th) for every (cur, last, th) of jobs (distinct current frames),
    one search per job, every candidate whose point the arrays can express sent, and per search the last frame's
    indices of its items."""
    frames, blocked, rows, descs, items, levels, where, ths, modes = [], [], [], [], [], [], [], [], []
    f32 = False
    for cur, last, th in jobs:
        frames.append(pack_frame(cur))
        f32 = f32 or frames[-1]["f32"]
        blocked.append([1 if (m and m.observations() > 0) else 0 for m in cur.mvpMapPoints])
        pos, it, lv = [], [], []
        for i in range(last.N):
            p = last.mvpMapPoints[i]
            if p and not last.mvbOutlier[i] and expressible(p):
                w = p.get_world_pos()
                pos.append(i), it.append(len(rows)), lv.append(last.mvKeys[i].octave)
                rows.append([float(x) for x in w.reshape(-1)] + [float("nan")] * 6)
                descs.append(np.asarray(p.get_descriptor(), np.uint8).reshape(32))
                f32 = f32 or w.dtype == np.float32
        items.append(it), levels.append(lv), where.append(pos)
        ths.append(float(th)), modes.append(mode_of(cur, last))
    return join(frames, blocked, rows, descs, ths, modes, list(range(len(jobs))), items, levels,
                EPS_F32 if f32 else EPS_F64), where


# ---- the reference's bodies on the objects ----------------------------------------------------------------------------

def ff_one(cur, last, i, pMP, th, mode):
    """ORBMatcher.py:314-367 for one candidate of the last frame against the current frame's current slots, statement
    by statement on the stand-in objects, so every dtype promotion is the reference's: (best_dist, best_idx2)."""
    Rcw = cur.mTcw[:3, :3]
    tcw = cur.mTcw[:3, 3:4]
    with np.errstate(all="ignore"):
        x3Dw = pMP.get_world_pos()
        x3Dc = Rcw @ x3Dw + tcw
        xc, yc, zc = x3Dc[0][0], x3Dc[1][0], x3Dc[2][0]
        invzc = 1.0 / zc
        if invzc < 0:
            return 256, -1
        u = cur.fx * xc * invzc + cur.cx
        v = cur.fy * yc * invzc + cur.cy
        if u < cur.mnMinX or u > cur.mnMaxX:
            return 256, -1
        if v < cur.mnMinY or v > cur.mnMaxY:
            return 256, -1
        n_last_octave = last.mvKeys[i].octave
        radius = th * cur.mvScaleFactors[n_last_octave]
        if mode == 1:
            v_indices2 = cur.get_features_in_area(u, v, radius, n_last_octave, -1)
        elif mode == 2:
            v_indices2 = cur.get_features_in_area(u, v, radius, 0, n_last_octave)
        else:
            v_indices2 = cur.get_features_in_area(u, v, radius, n_last_octave - 1, n_last_octave + 1)
        best_dist, best_idx2 = 256, -1
        if not v_indices2:
            return best_dist, best_idx2
        dMP = pMP.get_descriptor()
        for i2 in v_indices2:
            if cur.mvpMapPoints[i2]:
                if cur.mvpMapPoints[i2].observations() > 0:
                    continue
            if cur.mvuRight[i2] > 0:
                ur = u - cur.mbf * invzc
                er = abs(ur - cur.mvuRight[i2])
                if er > radius:
                    continue
            dist = O.popcount(dMP, cur.mDescriptors[i2])
            if dist < best_dist:
                best_dist = dist
                best_idx2 = i2
    return best_dist, best_idx2


class _Tally:
    """The assignment, the count and the rotation histogram with its rejection (ORBMatcher.py:370-391)."""

    def __init__(self, cur, last, check_ori):
        self.cur, self.last, self.check_ori = cur, last, check_ori
        self.n, self.hist, self.twice, self.mine = 0, [[] for _ in range(HISTO_LENGTH)], 0, set()

    def assign(self, i, pMP, best_idx2):
        self.twice += int(best_idx2 in self.mine)  # a point without observations is overwritten
        self.mine.add(best_idx2)
        self.cur.mvpMapPoints[best_idx2] = pMP
        self.n += 1
        if self.check_ori:
            rot = self.last.mvKeysUn[i].angle - self.cur.mvKeysUn[best_idx2].angle
            if rot < 0.0:
                rot += 360.0
            b = round(rot * (1.0 / HISTO_LENGTH))
            if b == HISTO_LENGTH:
                b = 0
            assert 0 <= b < HISTO_LENGTH
            self.hist[b].append(best_idx2)

    def finish(self):
        if self.check_ori:
            keep = [int(k) for k in three_maxima([len(h) for h in self.hist])]
            for b in range(HISTO_LENGTH):
                if b not in keep:
                    for idx in self.hist[b]:
                        self.cur.mvpMapPoints[idx] = None
                        self.n -= 1
        return self.n


def loop(cur, last, th, check_ori=True, stats=None):
    """ORBMatcher.search_by_projection_f_f on the stand-in objects, body by body."""
    mode = mode_of(cur, last)
    t = _Tally(cur, last, check_ori)
    for i in range(last.N):
        pMP = last.mvpMapPoints[i]
        if pMP:
            if not last.mvbOutlier[i]:
                best_dist, best_idx2 = ff_one(cur, last, i, pMP, th, mode)
                if best_dist <= TH_HIGH:
                    t.assign(i, pMP, best_idx2)
    if stats is not None:
        stats["twice"] = stats.get("twice", 0) + t.twice
    return t.finish()


def _taken(F, idx):
    m = F.mvpMapPoints[idx]
    return bool(m) and m.observations() > 0


def replay(jobs, results=None, stats=None, check_ori=True):
    """[search_by_projection_f_f(cur, last, th) for (cur, last, th) in jobs] from array results over pack(jobs) taken
    BEFORE the first assignment (None: computed here with search; a callable: called with the arrays).  In list order:
    a marked item, an item whose point the arrays cannot express and an item whose best feature a point with
    observations has taken meanwhile are redone by ff_one against the current slots; the others stand.  stats counts the
    items sent (items), the marked ones (marginal), those redone because their feature was taken (taken), those not
    expressible (alone), the features assigned twice (twice) and every ff_one call as its (search, last-frame index)
    (redone)."""
    a, where = pack(jobs)
    if results is None or callable(results):
        results = (results or search)(a)
    res = dict(zip(OUTPUTS, results))
    stats = {} if stats is None else stats
    for key in ("items", "marginal", "taken", "alone", "twice"):
        stats.setdefault(key, 0)
    stats.setdefault("redone", [])
    out = []
    for s, (cur, last, th) in enumerate(jobs):
        mode = int(a["srch_mode"][s])
        at = {i: int(a["srch_off"][s]) + c for c, i in enumerate(where[s])}
        t = _Tally(cur, last, check_ori)
        for i in range(last.N):
            pMP = last.mvpMapPoints[i]
            if not (pMP and not last.mvbOutlier[i]):
                continue
            j = at.get(i)
            redo = j is None
            if j is None:
                stats["alone"] += 1
            else:
                stats["items"] += 1
                bi, bd = int(res["best_idx"][j]), int(res["best_dist"][j])
                if res["status"][j]:
                    stats["marginal"] += 1
                    redo = True
                elif bi < 0 or bd > TH_HIGH:
                    continue
                elif _taken(cur, bi):
                    stats["taken"] += 1
                    redo = True
            if redo:
                stats["redone"].append((s, i))
                bd, bi = ff_one(cur, last, i, pMP, th, mode)
            if bd <= TH_HIGH:
                t.assign(i, pMP, bi)
        stats["twice"] += t.twice
        out.append(t.finish())
    return out
