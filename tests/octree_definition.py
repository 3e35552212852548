"""DistributeOctTree (ORBextractor.cpp:539-762) restated on Python lists, with an optional trace of every decision
it takes, and the two depths the host derives for k_octree_bins (orbfe_host.hip octree_tables).

The definition is what tests/test_oracle_cpu.py holds the oracle to; the trace is what tests/octree_cases.py
classifies its placements by (which pass the list ends on, the careful switch's operands, the break, the tie runs,
the depths divided and kept, the equal maxima of a final node).  The trace never changes the result."""
from __future__ import annotations

import math

import numpy as np


class _Node:
    __slots__ = ("keys", "x0", "y0", "x1", "y1", "nomore", "cid", "depth", "path")


class CarefulIteration:
    """One iteration of the careful phase.

    candidates  the nodes to divide, in the order they are taken (largest first; equal sizes by creation id):
                (size, creation id, depth, non-empty children)
    divided     how many of them were divided (all of them unless the list reached N)
    broke       the list reached N inside the iteration
    length      the list length when the iteration ended
    runs        every run of >= 2 equal-size candidates: (size, first position, length, straddles), straddles =
                the break fell inside the run (some of its nodes divided, some not)"""

    def __init__(self):
        self.candidates, self.divided, self.broke, self.length, self.runs = [], 0, False, 0, []
        self.paths = []  # per candidate: (initial column, quadrant at depth 1, quadrant at depth 2, ...)


class Trace:
    """full_passes    number of full passes
    switch_tests   (S, nexp, N) at every evaluation of S + 3 nexp > N (one per full pass that neither reached N nor
                   stopped growing)
    pass_lengths   the list length after every full pass
    pass_depths    per full pass, the depths of the nodes it divided
    pass_paths     per full pass, the paths of the nodes it divided (see CarefulIteration.paths)
    full_end       how the full passes ended: 'reached N', 'no growth' or 'careful'
    careful        the CarefulIteration list
    careful_end    'break' (reached N inside an iteration), 'no growth' (an iteration added nothing) or None
    divided_depths the depth of every divided node, in division order
    divided_boxes  its box (x0, y0, x1, y1)
    divided_keys   its key indices
    final          per final node, in list order: (depth, size, the key indices sharing its maximum response, its
                   first key index, its last)"""

    def __init__(self):
        self.full_passes, self.switch_tests, self.pass_lengths, self.pass_depths = 0, [], [], []
        self.pass_paths, self.divided_boxes, self.divided_keys = [], [], []
        self.full_end, self.careful, self.careful_end = None, [], None
        self.divided_depths, self.final = [], []


def n_ini(span_x: int, span_y: int) -> int:
    return int(math.floor(np.float32(span_x) / np.float32(span_y) + np.float32(0.5)))


def column_width(span_x: int, span_y: int) -> np.float32:
    return np.float32(np.float32(span_x) / np.float32(n_ini(span_x, span_y)))


def column_of(x: int, hX: np.float32) -> int:
    return int(np.float32(np.float32(x) / hX))


def column_box(i: int, hX: np.float32) -> tuple:
    return int(np.float32(hX * np.float32(i))), int(np.float32(hX * np.float32(i + 1)))


def octree_py(K, minX, maxX, minY, maxY, N, reverse_ties=False, trace: Trace | None = None):
    """DistributeOctTree on a Python list; ties by creation id (the careful phase divides the most recently
    created of equal-size nodes first), or with reverse_ties the oldest first — a second admissible heap-address
    order."""
    if not K:
        return []
    nIni = n_ini(maxX - minX, maxY - minY)
    hX = column_width(maxX - minX, maxY - minY)
    ctr = [0]

    def mk(keys, x0, y0, x1, y1, depth, path):
        n = _Node()
        n.keys, n.x0, n.y0, n.x1, n.y1, n.nomore = keys, x0, y0, x1, y1, len(keys) == 1
        n.cid, n.depth, n.path = ctr[0], depth, path
        ctr[0] += 1
        return n

    ini = [mk([], column_box(i, hX)[0], 0, column_box(i, hX)[1], maxY - minY, 0, (i,)) for i in range(nIni)]
    for i, k in enumerate(K):
        ini[column_of(k[0], hX)].keys.append(i)
    nodes = []
    for n in ini:
        if n.keys:
            n.nomore = len(n.keys) == 1
            nodes.append(n)

    def divide(n):
        hx, hy = (n.x1 - n.x0 + 1) // 2, (n.y1 - n.y0 + 1) // 2
        mx, my = n.x0 + hx, n.y0 + hy
        parts = [[], [], [], []]
        for i in n.keys:
            parts[(0 if K[i][0] < mx else 1) + (0 if K[i][1] < my else 2)].append(i)
        boxes = [(n.x0, n.y0, mx, my), (mx, n.y0, n.x1, my), (n.x0, my, mx, n.y1), (mx, my, n.x1, n.y1)]
        if trace is not None:
            trace.divided_depths.append(n.depth)
            trace.divided_boxes.append((n.x0, n.y0, n.x1, n.y1))
            trace.divided_keys.append(n.keys)
        return [(parts[q], boxes[q], n.path + (q,)) for q in range(4)]

    def children(n):
        hx, hy = (n.x1 - n.x0 + 1) // 2, (n.y1 - n.y0 + 1) // 2
        mx, my = n.x0 + hx, n.y0 + hy
        return len({(K[i][0] >= mx, K[i][1] >= my) for i in n.keys})

    while True:
        prev = len(nodes)
        front, keep, expand = [], [], []
        depths, paths = [], []
        for n in nodes:
            if n.nomore:
                keep.append(n)
                continue
            depths.append(n.depth)
            paths.append(n.path)
            for keys, b, path in divide(n):
                if keys:
                    c = mk(keys, *b, n.depth + 1, path)
                    front.insert(0, c)
                    if len(keys) > 1:
                        expand.append(c)
        nodes = front + keep
        if trace is not None:
            trace.full_passes += 1
            trace.pass_lengths.append(len(nodes))
            trace.pass_depths.append(depths)
            trace.pass_paths.append(paths)
        if len(nodes) >= N or len(nodes) == prev:
            if trace is not None:
                trace.full_end = "reached N" if len(nodes) >= N else "no growth"
            break
        if trace is not None:
            trace.switch_tests.append((len(nodes), len(expand), N))
        if len(nodes) + 3 * len(expand) > N:
            if trace is not None:
                trace.full_end = "careful"
            while True:
                prev = len(nodes)
                todo = sorted(expand, key=lambda n: (len(n.keys), -n.cid if reverse_ties else n.cid))
                expand = []
                done = False
                it = CarefulIteration()
                it.candidates = [(len(n.keys), n.cid, n.depth, children(n)) for n in reversed(todo)]
                it.paths = [n.path for n in reversed(todo)]
                for n in reversed(todo):
                    kids = []
                    for keys, b, path in divide(n):
                        if keys:
                            c = mk(keys, *b, n.depth + 1, path)
                            kids.insert(0, c)
                            if len(keys) > 1:
                                expand.append(c)
                    nodes.remove(n)
                    nodes = kids + nodes
                    it.divided += 1
                    if len(nodes) >= N:
                        done = True
                        break
                if trace is not None:
                    it.broke, it.length = done, len(nodes)
                    a = 0
                    while a < len(it.candidates):
                        b = a
                        while b < len(it.candidates) and it.candidates[b][0] == it.candidates[a][0]:
                            b += 1
                        if b - a >= 2:
                            it.runs.append((it.candidates[a][0], a, b - a, done and a < it.divided < b))
                        a = b
                    trace.careful.append(it)
                if done or len(nodes) >= N or len(nodes) == prev:
                    if trace is not None:
                        trace.careful_end = "break" if done or len(nodes) >= N else "no growth"
                    break
            break
    out = []
    for n in nodes:
        best = n.keys[0]
        for i in n.keys[1:]:
            if K[i][2] > K[best][2]:
                best = i
        out.append(K[best])
        if trace is not None:
            trace.final.append((n.depth, len(n.keys), [i for i in n.keys if K[i][2] == K[best][2]], n.keys[0],
                                n.keys[-1]))
    return out


def bin_depths(span_x: int, span_y: int, N: int) -> tuple:
    """(D, D0) of a level as octree_tables derives them.  D: the least depth at which neighbouring pixels of a
    column (and neighbouring rows) differ in their halving path, over the coordinates a key can take
    (x_rel < span_x - 3, y_rel < span_y - 3).  D0: the least depth >= 1 with nIni 4^D0 >= 8 N, capped by D and
    lowered while nIni 4^D0 > 2048."""
    nIni, hX = n_ini(span_x, span_y), column_width(span_x, span_y)

    def path(v, lo, hi):
        bits = []
        for _ in range(15):
            m = lo + (hi - lo + 1) // 2
            bits.append(v >= m)
            lo, hi = (m, hi) if v >= m else (lo, m)
        return bits

    def split(a, b):
        return 1 + next(d for d in range(15) if a[d] != b[d])

    col = [min(column_of(x, hX), nIni - 1) for x in range(span_x + 1)]
    xp = [path(x, *column_box(col[x], hX)) for x in range(span_x + 1)]
    yp = [path(y, 0, span_y) for y in range(span_y + 1)]
    D = 1
    for x in range(1, max(1, span_x - 3)):
        if col[x] == col[x - 1]:
            D = max(D, split(xp[x], xp[x - 1]))
    for y in range(1, max(1, span_y - 3)):
        D = max(D, split(yp[y], yp[y - 1]))
    D0 = 1
    while D0 < D and nIni << (2 * D0) < 8 * max(N, 1):
        D0 += 1
    while D0 > 1 and nIni << (2 * D0) > 2048:
        D0 -= 1
    return D, D0
