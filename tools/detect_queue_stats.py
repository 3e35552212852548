"""Per-cell queue sizes of k_detect's two-queue path on synthetic KITTI images (numpy restatement of the
pre-test bound, the exact FAST M and the NMS; tools only, not a test): how many 64-lane M / NMS steps each
stage runs, and what a B \\ A fallback queue would save; and what k_detect's lanes do per
cell (lane_counts): the B entries that the idle lanes of A's last M step carry, the pre-test halves without a live
row and the halves without an A pair (the counters of orbfe_debug_detect_lanes)."""
import sys

import numpy as np

sys.path.insert(0, ".")
from oracle.oracle import OracleExtractor  # noqa: E402
from pyorbslam_amd import synth  # noqa: E402

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
          (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def maps(img):
    I = img.astype(np.int32)
    h, w = I.shape
    P = np.pad(I, 3, mode="edge")
    d = np.stack([I - P[3 + dy:3 + dy + h, 3 + dx:3 + dx + w] for dx, dy in CIRCLE])  # (16, h, w)
    M = np.zeros((h, w), np.int32)
    for k in range(16):
        idx = [(k + j) % 16 for j in range(9)]
        M = np.maximum(M, d[idx].min(0))
        M = np.maximum(M, (-d[idx]).min(0))
    c = [P[3 + dy:3 + dy + h, 3 + dx:3 + dx + w] for dx, dy in ((0, 3), (3, 0), (0, -3), (-3, 0))]
    a = np.maximum(np.minimum(c[0], c[2]), np.minimum(c[1], c[3]))
    b = np.minimum(np.maximum(c[0], c[2]), np.maximum(c[1], c[3]))
    bound = np.maximum(I - a, b - I)
    return M, bound


def cells(w, h):
    minX, minY, maxX, maxY = 16, 16, w - 16, h - 16
    W, H = maxX - minX, maxY - minY
    nC, nR = int(W / 30.0), int(H / 30.0)
    if nC <= 0 or nR <= 0:
        return
    wC, hC = int(np.ceil(W / nC)), int(np.ceil(H / nR))
    for i in range(nR):
        y0 = minY + i * hC
        if y0 >= maxY - 3:
            continue
        y1 = min(y0 + hC + 6, maxY)
        for j in range(nC):
            x0 = minX + j * wC
            if x0 >= maxX - 6:
                continue
            x1 = min(x0 + wC + 6, maxX)
            yield x0, y0, x1, y1


def pair_cap(cell):
    """The cell's pair count, rounded up to 8; Geo::fd_pq is the largest of a geometry."""
    ww, wh = max(cell[2] - cell[0] - 6, 0), max(cell[3] - cell[1] - 6, 0)
    return (((ww + 1) // 2) * wh + 7) & ~7


def pair_maps(M, bound, cell):
    """(pm, pb): the larger M / bound of each horizontal pixel pair of the cell's window, (wh, ceil(ww / 2)); the
    pixel right of an odd window counts 0, as in the kernel."""
    x0, y0, x1, y1 = cell
    ww, wh = x1 - x0 - 6, y1 - y0 - 6
    pw = (ww + 1) // 2
    Mp = np.zeros((wh, 2 * pw), np.int32)
    Bp = np.zeros((wh, 2 * pw), np.int32)
    Mp[:, :ww] = M[y0 + 3:y0 + 3 + wh, x0 + 3:x0 + 3 + ww]
    Bp[:, :ww] = bound[y0 + 3:y0 + 3 + wh, x0 + 3:x0 + 3 + ww]
    return np.maximum(Mp[:, 0::2], Mp[:, 1::2]), np.maximum(Bp[:, 0::2], Bp[:, 1::2])


def lane_counts(M, bound, cell, cap, ini=20, mn=7):
    """What k_detect does with one cell when minTh < iniTh: the queue lengths, the path, and the counters of
    orbfe_debug_detect_lanes (a_skipped counts the halves the kernel runs, an empty second half included).  cap = the largest cell's pair count of the geometry (Geo::fd_pq)."""
    x0, y0, x1, y1 = cell
    ww, wh = x1 - x0 - 6, y1 - y0 - 6
    pm, pb = pair_maps(M, bound, cell)
    A, B = pb > ini, pb > mn
    nA, nB = int(A.sum()), int(B.sum())
    Mw = M[y0 + 3:y0 + 3 + wh, x0 + 3:x0 + 3 + ww]
    Z = np.pad(Mw, 1)
    nb = np.max([Z[1 + dy:1 + dy + wh, 1 + dx:1 + dx + ww] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx],
                axis=0)
    kept_ini = int(((Mw > max(ini, 1)) & (Mw > nb)).sum())
    # pre-test halves of 64 quads (4 px): rows of 8 lanes while a row has at most 8 quads, else row-major quads
    qrow = (ww + 3) >> 2
    qa = np.zeros((wh, 2 * qrow), bool)
    qa[:, :A.shape[1]] = A
    qa = qa[:, 0::2] | qa[:, 1::2]                                      # quads with an A pair
    if qrow <= 8:
        halves = [qa[r:r + 8].any() for r in range(0, wh, 8)]
    else:
        flat = qa.ravel()
        halves = [flat[i:i + 64].any() for i in range(0, flat.size, 64)]
    collide = nA + nB > cap
    fallback = not collide and kept_ini == 0
    kb = 0 if collide or nA == 0 else min(-nA % 64, nB)
    # the kernel runs two halves per iteration: halves_empty = 1 when the last one's second half has no live row
    return dict(ww=ww, wh=wh, qrow=qrow, A=nA, B=nB, collide=collide, fallback=fallback, kb=kb,
                carry_steps=int(kb > 0), b_steps=-(-(nB - kb) // 64) if fallback else 0,
                halves=len(halves), halves_empty=len(halves) & 1, a_halves=halves,
                a_skipped=sum(1 for h in halves if not h) + (len(halves) & 1),
                b_steps_saved=(-(-nB // 64) - -(-(nB - kb) // 64)) if fallback else 0)


def main(n_img=4, ini=20, mn=7):
    lanes(n_img, ini, mn)
    queues(n_img, ini, mn)


def lanes(n_img, ini, mn):
    """The three counts behind the idle-lane work: per cell, over left and right images."""
    st = dict(cells=0, fb=0, fb_with_A=0, m_steps_A=0, m_steps_B=0, b_steps_saved=0, halves_run=0, halves_needed=0,
              halves_without_A=0, wh_above_32=0)
    for s in range(n_img):
        for img in synth.make_pair(10_000 + s):
            o = OracleExtractor(iniThFAST=ini, minThFAST=mn)
            o.extract(img)
            pyr = o.pyramid()
            cap = max(pair_cap(c) for lvl in pyr for c in cells(lvl.shape[1], lvl.shape[0]))
            for lvl in pyr:
                M, bound = maps(lvl)
                for c in cells(lvl.shape[1], lvl.shape[0]):
                    if c[2] - c[0] <= 6 or c[3] - c[1] <= 6:
                        continue
                    r = lane_counts(M, bound, c, cap, ini, mn)
                    st["cells"] += 1
                    st["fb"] += r["fallback"]
                    st["fb_with_A"] += r["fallback"] and r["A"] > 0
                    st["m_steps_A"] += -(-r["A"] // 64)
                    st["m_steps_B"] += -(-r["B"] // 64) if r["fallback"] else 0
                    st["b_steps_saved"] += r["b_steps_saved"]
                    st["halves_run"] += r["halves"] + r["halves_empty"]      # two per iteration
                    st["halves_needed"] += r["halves"]
                    st["halves_without_A"] += r["a_skipped"] - r["halves_empty"]   # of the needed ones
                    st["wh_above_32"] += r["wh"] > 32
    c = st["cells"]
    print("lanes:", {k: round(v / c, 3) for k, v in st.items()}, "cells", c)


def queues(n_img=4, ini=20, mn=7):
    st = dict(cells=0, fb=0, A=0, B=0, stA=0, stB=0, stBp=0, nmsA=0, nmsB=0, nmsAmin=0, nnBp=0)
    hist = []
    for s in range(n_img):
        L, _ = synth.make_pair(10_000 + s)
        o = OracleExtractor()
        o.extract(L)
        for lvl in o.pyramid():
            M, bound = maps(lvl)
            for x0, y0, x1, y1 in cells(lvl.shape[1], lvl.shape[0]):
                wy0, wx0, ww, wh = y0 + 3, x0 + 3, x1 - x0 - 6, y1 - y0 - 6
                if ww <= 0 or wh <= 0:
                    continue
                Mw = M[wy0:wy0 + wh, wx0:wx0 + ww]
                Bw = bound[wy0:wy0 + wh, wx0:wx0 + ww]
                pw = (ww + 1) // 2
                Mp = np.zeros((wh, 2 * pw), np.int32)
                Bp = np.zeros((wh, 2 * pw), np.int32)
                Mp[:, :ww], Bp[:, :ww] = Mw, Bw
                pb = np.maximum(Bp[:, 0::2], Bp[:, 1::2])
                pm = np.maximum(Mp[:, 0::2], Mp[:, 1::2])
                A, B = pb > ini, pb > mn
                nA, nB = int(A.sum()), int(B.sum())
                # NMS at a threshold over the window (outside = 0)
                Z = np.pad(Mw, 1)
                nb = np.max([Z[1 + dy:1 + dy + wh, 1 + dx:1 + dx + ww] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                             if dy or dx], axis=0)
                kept_ini = int(((Mw > ini) & (Mw > nb)).sum())
                fb = kept_ini == 0
                st["cells"] += 1
                st["A"] += nA
                st["stA"] += -(-nA // 64)
                nnA = int((A & (pm > ini)).sum())
                st["nmsA"] += -(-nnA // 64)
                st["nmsAmin"] += -(-int((A & (pm > mn)).sum()) // 64)
                if fb:
                    st["fb"] += 1
                    st["B"] += nB
                    st["stB"] += -(-nB // 64)
                    st["stBp"] += -(-(nB - nA) // 64)
                    nnB = int((B & (pm > mn)).sum())
                    st["nmsB"] += -(-nnB // 64)
                    st["nnBp"] += -(-int((B & ~A & (pm > mn)).sum()) // 64)
                    hist.append((nA, nB))
    c = st["cells"]
    print({k: round(v / c, 3) for k, v in st.items()}, "cells", c)
    h = np.array(hist)
    print("fallback cells: mean |A|", h[:, 0].mean(), "mean |B|", h[:, 1].mean(),
          "share with |A| = 0:", (h[:, 0] == 0).mean())


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4)
