"""Array oracle of the BoW-guided match (ORBMatcher.search_by_BoW_kf_f / _kf_kf, ORBMatcher.py:21-213): the
loops as include/orbfe.h states them for k_bow_match, in plain Python over arrays, and the reference's
rotation rejection spelled with np.argsort as the reference spells it.  Test infrastructure only.

A frame is a dict: desc (n, 32) u8, angle (n,) f32, elig (n,) u8, fv_node (ascending), fv_end, fv_idx.
"""
from __future__ import annotations

import numpy as np

HISTO_LENGTH = 30


def hamming(a, b) -> int:
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def runs(f):
    """{node: [feature indices in run order]} in ascending node order."""
    out, a = {}, 0
    for node, e in zip(f["fv_node"].tolist(), f["fv_end"].tolist()):
        out[node] = f["fv_idx"][a:e].tolist()
        a = e
    return out


def match_pair(f1, f2, use_elig1=True, use_elig2=True, th=50, inclusive=False, nnratio=1.0, block=True):
    """(match12, match21, bin12, hist, n_raw) of one pair.  block=False drops the blocking of matched side-2
    features (only for showing that a case depends on it)."""
    n1, n2 = len(f1["desc"]), len(f2["desc"])
    match12 = np.full(n1, -1, np.int32)
    match21 = np.full(n2, -1, np.int32)
    bin12 = np.full(n1, -1, np.int8)
    hist = np.zeros(32, np.int32)
    n_raw = 0
    r1, r2 = runs(f1), runs(f2)
    factor = 1.0 / HISTO_LENGTH
    for node in r1:  # ascending; nodes in both vectors = the reference's merge walk
        if node not in r2:
            continue
        for i1 in r1[node]:
            if use_elig1 and not f1["elig"][i1]:
                continue
            best1, best_i2, best2 = 256, -1, 256
            for i2 in r2[node]:
                if use_elig2 and not f2["elig"][i2]:
                    continue
                if block and match21[i2] >= 0:
                    continue
                dist = hamming(f1["desc"][i1], f2["desc"][i2])
                if dist < best1:
                    best2 = best1
                    best1 = dist
                    best_i2 = i2
                elif dist < best2:
                    best2 = dist
            near = best1 <= th if inclusive else best1 < th
            if near and float(best1) < nnratio * float(best2):
                match12[i1] = best_i2
                match21[best_i2] = i1
                rot = float(f1["angle"][i1]) - float(f2["angle"][best_i2])
                if rot < 0.0:
                    rot += 360.0
                b = round(rot * factor)
                if b == HISTO_LENGTH:
                    b = 0
                bin12[i1] = b
                hist[b] += 1
                n_raw += 1
    return match12, match21, bin12, hist, n_raw


def three_maxima(hist):
    """ORBMatcher.compute_three_maxima over the bin counts, exactly as the reference spells it."""
    histo_counts = [int(c) for c in hist[:HISTO_LENGTH]]
    return np.argsort(histo_counts)[::-1][:3]


def reject(match12, match21, bin12, hist, n_raw, keep=None):
    """(match12, match21, n) after the reference's rotation rejection (ORBMatcher.py:108-116, 202-210)."""
    ind = three_maxima(hist) if keep is None else keep
    match12, match21 = match12.copy(), match21.copy()
    n = int(n_raw)
    for i1 in range(len(match12)):
        if match12[i1] >= 0 and int(bin12[i1]) not in [int(k) for k in ind]:
            match21[match12[i1]] = -1
            match12[i1] = -1
            n -= 1
    return match12, match21, n


def cut_is_stable(hist) -> bool:
    """The rotation cut does not hinge on how equal counts are ranked: the third and fourth largest counts
    differ, or the fourth is 0 (an empty bin holds no match to drop or keep)."""
    c = sorted((int(v) for v in hist[:HISTO_LENGTH]), reverse=True)
    return c[3] == 0 or c[2] != c[3]
