"""Array oracle of the triangulation match (ORBMatcher.search_for_triangulation, ORBMatcher.py:584-711): the walk,
the loops and the two gates as include/orbfe.h states them for k_tri_match, in plain Python over arrays.  It squares
with `** 2` on NumPy doubles, as the reference does.  Test infrastructure only.

A frame is a dict: desc (n, 32) u8, angle (n,) f32, xy (n, 2) f64, octave (n,) i32, flags (n,) u8 (bit 0: no map
point, bit 1: stereo), fv_node (ascending), fv_end, fv_idx, thr_epi (L,) f64, thr_ex (L,) f64.
"""
from __future__ import annotations

import numpy as np

from bow_match_oracle import HISTO_LENGTH, hamming, runs, three_maxima  # noqa: F401

ELIGIBLE, STEREO = 1, 2
MARGINAL = 1
MARGIN = 2.0 ** -48
MIN_NORMAL = 2.0 ** -1022


def walk(nodes1, nodes2):
    """The reference's walk (ORBMatcher.py:604-677) over two node lists: ([(r1, r2)] visited, stopped)."""
    out = []
    it1, it2 = iter(enumerate(nodes1)), iter(enumerate(nodes2))
    while True:
        try:
            r1, k1 = next(it1)
            r2, k2 = next(it2)
        except StopIteration:
            return out, False
        try:
            if k1 == k2:
                out.append((r1, r2))
            elif k1 < k2:
                next(it1)
            else:
                next(it2)
        except StopIteration:
            return [], True


def merge_common(nodes1, nodes2):
    """What a true merge would visit: the nodes both lists hold."""
    return sorted(set(nodes1) & set(nodes2))


def near(lhs, thr) -> bool:
    return bool(abs(lhs - thr) <= thr * MARGIN)


def match_pair(f1, f2, F12, ex, ey, th=50, only_stereo=False, block=True, use_ex=True, use_epi=True):
    """(match12, bin12, hist, n_raw, status, stopped) of one pair.  block / use_ex / use_epi = False drop the blocking
    of matched side-2 features / the epipole gate / the line test (only for showing that a case depends on them)."""
    n1 = len(f1["desc"])
    match12 = np.full(n1, -1, np.int32)
    bin12 = np.full(n1, -1, np.int8)
    hist = np.zeros(32, np.int32)
    n_raw, status = 0, 0
    vis, stopped = walk(f1["fv_node"].tolist(), f2["fv_node"].tolist())
    if stopped:
        return match12, bin12, hist, 0, 0, 1
    F12 = np.asarray(F12, np.float64).reshape(3, 3)
    ex, ey = np.float64(ex), np.float64(ey)
    r1, r2 = list(runs(f1).values()), list(runs(f2).values())
    need = ELIGIBLE | STEREO if only_stereo else ELIGIBLE
    taken = np.zeros(len(f2["desc"]), bool)
    factor = 1.0 / HISTO_LENGTH
    for v1, v2 in vis:
        for i1 in r1[v1]:
            if (f1["flags"][i1] & need) != need:
                continue
            x1, y1 = np.float64(f1["xy"][i1, 0]), np.float64(f1["xy"][i1, 1])
            a = x1 * F12[0, 0] + y1 * F12[1, 0] + F12[2, 0]
            b = x1 * F12[0, 1] + y1 * F12[1, 1] + F12[2, 1]
            c = x1 * F12[0, 2] + y1 * F12[1, 2] + F12[2, 2]
            den = a ** 2 + b ** 2
            best_d, best_i2 = th, -1
            for i2 in r2[v2]:
                if (f2["flags"][i2] & need) != need or (block and taken[i2]):
                    continue
                d = hamming(f1["desc"][i1], f2["desc"][i2])
                if d > th:
                    continue
                # the gates are evaluated for every such candidate (the kernel's marginal test sees them all); the
                # reference skips them when d > bestDist, which cannot change the winner
                x2, y2 = np.float64(f2["xy"][i2, 0]), np.float64(f2["xy"][i2, 1])
                o = int(f2["octave"][i2])
                if use_ex and not (f1["flags"][i1] & STEREO) and not (f2["flags"][i2] & STEREO):
                    e = (ex - x2) ** 2 + (ey - y2) ** 2
                    t = np.float64(f2["thr_ex"][o])
                    if near(e, t):
                        status |= MARGINAL
                    if e < t:
                        continue
                if use_epi:
                    if den == 0:
                        continue
                    if den < MIN_NORMAL:
                        status |= MARGINAL
                    num = a * x2 + b * y2 + c
                    q = (num ** 2) / den
                    t = np.float64(f2["thr_epi"][o])
                    if near(q, t):
                        status |= MARGINAL
                    if not q < t:
                        continue
                if d > best_d:
                    continue
                best_d, best_i2 = d, i2
            if best_i2 >= 0:
                match12[i1] = best_i2
                taken[best_i2] = True
                rot = float(f1["angle"][i1]) - float(f2["angle"][best_i2])
                if rot < 0:
                    rot += 360.0
                q = round(rot * factor)
                bn = q if 0 <= q <= HISTO_LENGTH else 31
                if bn == HISTO_LENGTH:
                    bn = 0
                if bn == 31:
                    status |= MARGINAL
                bin12[i1] = bn
                hist[bn] += 1
                n_raw += 1
    return match12, bin12, hist, n_raw, status, 0


def finish(match12, bin12, hist, check_ori, keep=None):
    """[(i1, i2)] after the reference's rotation rejection (ORBMatcher.py:679-696)."""
    ind = [int(k) for k in (three_maxima(hist) if keep is None else keep)]
    return [(i1, int(m)) for i1, m in enumerate(match12.tolist())
            if m >= 0 and (not check_ori or int(bin12[i1]) in ind)]


def cut_is_stable(hist) -> bool:
    c = sorted((int(v) for v in hist[:HISTO_LENGTH]), reverse=True)
    return c[3] == 0 or c[2] != c[3]
