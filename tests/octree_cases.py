"""Placements that put DistributeOctTree's decisions on their edges (tests/test_gpu_octree_edges.py) and the CPU
proof that they stand there (tests/test_octree_cases_cpu.py): deterministic, pure numpy plus the oracle.

A single pixel of value v on a flat background b is a FAST corner of score v - b - 1 and nothing near it is one;
with one level the level-0 target N equals nfeatures.  So an image hands the octree any candidate list
(x, y, response) and any N: dots of value 121 .. 255 on background 100 (or any value on background 0), no two
closer than 4 px in both axes, anywhere from pixel 19 to side - 20.  For a level above 0: scaleFactor 2, two
levels, 2 x 2 blocks of 255 at even positions (level 0 gets no candidate: the four pixels tie and the strict
non-maximum suppression drops them; level 1 gets one dot of score 154 per block at half the coordinates).

Every case is a recipe (a seeded generator of dots), N and the classes it was built for; a class is a predicate
over the trace of tests/octree_definition.py, so test_octree_cases_cpu.py can show that a case reaches its
classes, and that every class of CLASSES has a case.  The seeds and quotas below were searched for with the
predicates themselves; nothing here depends on what a kernel returns.

Classes of groups A - C come in two forms, [flat] (kp_cap <= 512: k_octree_bins<., true>, the all-thread passes)
and [lds] (kp_cap >= 513: wave 0's LDS-list passes).  LDS_OUT_OF_REACH lists the [lds] forms no image of this
construction can hold, with the reason.  Two classes of the octree are out of this construction's reach in
either form and have no entry: a final node at depth D (a node of depth D - 1 is 2 px wide, dots stand 4 px apart),
and candidates of different depths in one careful iteration (an iteration's candidates are the children of the
previous iteration's divided nodes, so they always share a depth)."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import octree_definition as OD
from oracle import oracle as O

BG = 100
EDGE = 19           # FAST keeps corners in 19 <= x <= w - 20
BORDER = 16         # the octree's minX / minY
PITCH = 4
GEOS = {"sq": (130, 130), "two": (190, 100), "three": (240, 100), "four": (300, 100), "odd": (131, 97), "big": (400, 200)}
BASE = dict(scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7)
FLAT_MAX_CAP = 512  # octree_reg_passes: max_ncap <= 64 * 8


def params(N: int, nlevels: int = 1) -> dict:
    return dict(BASE, nfeatures=int(N), nlevels=nlevels, scaleFactor=2.0 if nlevels == 2 else 1.2)


# ---- recipes: each returns a list of (px, py, value) in level pixels ---------------------------------------------
def _free(occ, x, y):
    return not occ[max(0, y - PITCH + 1):y + PITCH, max(0, x - PITCH + 1):x + PITCH].any()


def scatter(w, h, seed, K, box=None, lo=121, hi=254, occ=None):
    """K dots at random free positions of box = (x0, y0, x1, y1) (inclusive, level pixels; the whole level by
    default), no two closer than PITCH in both axes."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = box or (EDGE, EDGE, w - EDGE - 1, h - EDGE - 1)
    occ = np.zeros((h, w), bool) if occ is None else occ
    out = []
    for _ in range(200 * K):
        if len(out) == K:
            break
        x, y = int(rng.integers(x0, x1 + 1)), int(rng.integers(y0, y1 + 1))
        if _free(occ, x, y):
            occ[y, x] = True
            out.append((x, y, int(rng.integers(lo, hi + 1))))
    assert len(out) == K, (len(out), K)
    return out


def clusters(w, h, seed, n_clusters, per, side, singles):
    """n_clusters patches of side x side px with `per` dots each, then `singles` dots anywhere."""
    rng = np.random.default_rng(seed)
    occ = np.zeros((h, w), bool)
    out = []
    for c in range(n_clusters):
        cx = int(rng.integers(EDGE, w - EDGE - side + 1))
        cy = int(rng.integers(EDGE, h - EDGE - side + 1))
        out += scatter(w, h, int(rng.integers(1 << 30)), per, (cx, cy, cx + side - 1, cy + side - 1), occ=occ)
    return out + (scatter(w, h, int(rng.integers(1 << 30)), singles, occ=occ) if singles else [])


def lattice(w, h, pitch=PITCH):
    return [(x, y) for y in range(EDGE, h - EDGE, pitch) for x in range(EDGE, w - EDGE, pitch)]


def node_path(w, h, x, y, depth):
    """The node of depth `depth` that holds level pixel (x, y): (column, quadrant, quadrant, ...)."""
    sx, sy = w - 2 * BORDER, h - 2 * BORDER
    hX = OD.column_width(sx, sy)
    xr, yr = x - BORDER, y - BORDER
    c = min(OD.column_of(xr, hX), OD.n_ini(sx, sy) - 1)
    (x0, x1), y0, y1 = OD.column_box(c, hX), 0, sy
    path = [c]
    for _ in range(depth):
        mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
        path.append((xr >= mx) + 2 * (yr >= my))
        x0, x1 = (mx, x1) if xr >= mx else (x0, mx)
        y0, y1 = (my, y1) if yr >= my else (y0, my)
    return tuple(path)


def quota(w, h, seed, depth, counts, fill=None):
    """The PITCH lattice thinned so that the nodes of depth `depth`, in path order, hold counts[0], counts[1], ...
    dots at most (`fill` for the nodes beyond the list; None = all of theirs)."""
    rng = np.random.default_rng(seed)
    by_node = {}
    for x, y in lattice(w, h):
        by_node.setdefault(node_path(w, h, x, y, depth), []).append((x, y))
    out = []
    for i, path in enumerate(sorted(by_node)):
        pts = by_node[path]
        n = counts[i] if i < len(counts) else (len(pts) if fill is None else fill)
        n = min(n, len(pts))
        keep = sorted(rng.permutation(len(pts))[:n].tolist())
        out += [pts[k] + (int(rng.integers(121, 255)),) for k in keep]
    return out


def sprinkle(w, h, seed, depth, base, specials=()):
    """quota() with drawn counts: every node of depth `depth` gets a count drawn from `base`, then, for every
    (m, lo, hi) of `specials`, m further nodes (disjoint) get one drawn from lo .. hi."""
    rng = np.random.default_rng(seed)
    n = len({node_path(w, h, x, y, depth) for x, y in lattice(w, h)})
    counts = rng.choice(base, n).tolist()
    order, at = rng.permutation(n), 0
    for m, lo, hi in specials:
        for k in order[at:at + m]:
            counts[k] = int(rng.integers(lo, hi + 1))
        at += m
    return quota(w, h, int(rng.integers(1 << 30)), depth, counts, 0)


def full_quads(w, h, seed, depth, a, b):
    """b nodes of depth `depth` with four non-empty children, of which one holds four dots that its own division
    sends to four children and three hold one dot; then a nodes of that depth with one dot."""
    rng = np.random.default_rng(seed)
    tree = {}
    for x, y in lattice(w, h):
        p = node_path(w, h, x, y, depth + 2)
        tree.setdefault(p[:-2], {}).setdefault(p[:-1], {}).setdefault(p, (x, y))
    full = [n for n in sorted(tree) if len(tree[n]) == 4 and any(len(c) == 4 for c in tree[n].values())]
    rest = sorted(tree)
    out = []
    for k in rng.permutation(len(full))[:b]:
        kids = tree[full[k]]
        rest.remove(full[k])
        quad = next(c for c in sorted(kids) if len(kids[c]) == 4)
        out += [kids[c][g] for c in sorted(kids) for g in (sorted(kids[c]) if c == quad else sorted(kids[c])[:1])]
    assert len(out) == 7 * b, (len(full), b)
    for k in rng.permutation(len(rest))[:a]:
        kids = tree[rest[k]]
        c = sorted(kids)[0]
        out.append(kids[c][sorted(kids[c])[0]])
    return [pt + (int(rng.integers(121, 255)),) for pt in out]


def patch(w, h, seed, x0, y0, nx, ny, singles=0):
    """The full PITCH lattice of nx x ny dots from level pixel (x0, y0), then `singles` dots anywhere."""
    rng = np.random.default_rng(seed)
    occ = np.zeros((h, w), bool)
    out = [(x0 + PITCH * i, y0 + PITCH * j, int(rng.integers(121, 255))) for j in range(ny) for i in range(nx)]
    for x, y, _ in out:
        occ[y, x] = True
    return out + (scatter(w, h, int(rng.integers(1 << 30)), singles, occ=occ) if singles else [])


def mixed(w, h, seed, dots, K, lo=121, hi=254):
    """The given dots (x, y, value), then K scattered ones."""
    occ = np.zeros((h, w), bool)
    for x, y, _ in dots:
        assert _free(occ, x, y), (x, y)
        occ[y, x] = True
    return [tuple(d) for d in dots] + (scatter(w, h, seed, K, None, lo, hi, occ) if K else [])


RECIPES = dict(scatter=scatter, clusters=clusters, quota=quota, sprinkle=sprinkle, full_quads=full_quads, patch=patch, mixed=mixed)


# ---- a case --------------------------------------------------------------------------------------------------------
def cell_order(w, h, dots):
    """The dots in the order the FAST cell grid yields them (ORBextractor.cpp:772-824): cells of about 30 px row by
    row, raster order inside a cell."""
    width, height = w - 2 * BORDER, h - 2 * BORDER
    wc = math.ceil(width / int(width / 30.0))
    hc = math.ceil(height / int(height / 30.0))
    return sorted(dots, key=lambda d: ((d[1] - EDGE) // hc, (d[0] - EDGE) // wc, d[1], d[0]))


def image_of(w, h, dots, bg=BG):
    img = np.full((h, w), bg, np.uint8)
    for x, y, v in dots:
        img[y, x] = v
    return img


class Case(NamedTuple):
    name: str
    geo: str
    recipe: str
    args: tuple
    N: int
    classes: tuple
    bg: int = BG
    level: int = 0      # 1: the dots are level-1 pixels of a two-level extractor (scaleFactor 2); N = nfeatures

    @property
    def size(self):
        w, h = GEOS[self.geo]
        return (2 * w, 2 * h) if self.level else (w, h)     # of the image

    @property
    def level_size(self):
        return GEOS[self.geo]

    @property
    def params(self):
        return params(self.N, 2 if self.level else 1)


@functools.lru_cache(maxsize=None)
def dots_of(case: Case) -> tuple:
    w, h = case.level_size
    return tuple(cell_order(w, h, RECIPES[case.recipe](w, h, *case.args)))


@functools.lru_cache(maxsize=None)
def image(case: Case) -> np.ndarray:
    w, h = case.level_size
    if not case.level:
        img = image_of(w, h, dots_of(case), case.bg)
    else:
        img = np.full((2 * h, 2 * w), BG, np.uint8)
        for x, y, _ in dots_of(case):
            img[2 * y:2 * y + 2, 2 * x:2 * x + 2] = 255
    img.setflags(write=False)
    return img


def placed(case: Case) -> list:
    """The candidate list the image promises, in key order: (x - 16, y - 16, v - bg - 1)."""
    if case.level:
        return [(x - BORDER, y - BORDER, 154) for x, y, _ in dots_of(case)]
    return [(x - BORDER, y - BORDER, v - case.bg - 1) for x, y, v in dots_of(case)]


def level_target(case: Case) -> int:
    """N of the case's level."""
    if not case.level:
        return case.N
    return int(O.OracleExtractor(**case.params).tables()["n_per_level"][1])


def kp_cap(n_ini: int, N: int) -> int:
    return max(N + 2, 4 * n_ini) + 2


def key_table_cap(NC: int) -> int:
    """Keys whose cells k_octree_bins keeps one by one: the u16 that fit the node-list region of its LDS carve
    (ob_carve entries 3 .. 16, each rounded to 16 bytes)."""
    al = lambda v: (v + 15) & ~15
    big = max(NC, 512)
    return (4 * al(4 * NC) + 2 * al(NC) + 4 * al(4 * NC) + al(8 * big) + al(8 * NC) + al(4 * NC) + al(NC)) // 2


class Info:
    """A case's trace and the level facts the predicates read."""

    def __init__(self, case: Case):
        w, h = case.level_size
        self.case, self.K, self.N = case, placed(case), level_target(case)
        self.sx, self.sy = w - 2 * BORDER, h - 2 * BORDER
        self.n_ini = OD.n_ini(self.sx, self.sy)
        self.hX = OD.column_width(self.sx, self.sy)
        self.D, self.D0 = OD.bin_depths(self.sx, self.sy, self.N)
        self.tr = OD.Trace()
        self.kept = OD.octree_py(self.K, BORDER, w - BORDER, BORDER, h - BORDER, self.N, trace=self.tr)
        self.columns = sorted({min(OD.column_of(k[0], self.hX), self.n_ini - 1) for k in self.K})
        if case.level:
            n0 = int(O.OracleExtractor(**case.params).tables()["n_per_level"][0])
            self.max_ncap = max(kp_cap(self.n_ini, self.N), kp_cap(OD.n_ini(2 * w - 32, 2 * h - 32), n0))
        else:
            self.max_ncap = kp_cap(self.n_ini, self.N)
        self.form = "flat" if self.max_ncap <= FLAT_MAX_CAP else "lds"

    @functools.cached_property
    def kept_reversed(self):
        w, h = self.case.level_size
        return OD.octree_py(self.K, BORDER, w - BORDER, BORDER, h - BORDER, self.N, reverse_ties=True)

    # the nodes with >= 2 keys a sweep over the keys counts the children of: per full pass and careful iteration
    def deep_sweeps(self):
        out = [[p for p in paths if len(p) - 1 >= self.D0] for paths in self.tr.pass_paths]
        out += [[p for p in it.paths if len(p) - 1 >= self.D0] for it in self.tr.careful]
        return [s for s in out if s]


@functools.lru_cache(maxsize=None)
def info(case: Case) -> Info:
    return Info(case)


# ---- the classes -----------------------------------------------------------------------------------------------------
def _last(i):
    return i.tr.careful[-1] if i.tr.careful else None


def _broke(i):
    return i.tr.careful_end == "break" and _last(i).broke


def _switch(i, k, first):
    """S + 3 nexp == N + k at the first pass's test, or at a later one (k = 1: the test that switched)."""
    t = i.tr.switch_tests
    idx = [j for j, (S, e, N) in enumerate(t) if S + 3 * e == N + k and (k == 0 or j == len(t) - 1)]
    if k == 1 and i.tr.full_end != "careful":
        return False
    return any((j == 0) == first for j in idx)


def _run(i, pred):
    return _broke(i) and any(pred(r) for r in _last(i).runs)


def _max_size(i, v):
    return any(it.candidates and it.candidates[0][0] == v for it in i.tr.careful)


def _M(i, m):
    return any(len(it.candidates) == m for it in i.tr.careful)


def _split_edges(i, odd):
    """A divided node with a box of odd (even) width holds keys at x == mx and x == mx - 1, and one of odd (even)
    height holds keys at y == my and y == my - 1."""
    okx = oky = False
    for (x0, y0, x1, y1), keys in zip(i.tr.divided_boxes, i.tr.divided_keys):
        mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
        xs, ys = {i.K[k][0] for k in keys}, {i.K[k][1] for k in keys}
        okx |= (x1 - x0) % 2 == odd and mx in xs and mx - 1 in xs
        oky |= (y1 - y0) % 2 == odd and my in ys and my - 1 in ys
    return okx and oky


def _raster_disagrees(i):
    for _, _, tied, *_ in i.tr.final:
        if len(tied) >= 2:
            first = min(tied, key=lambda k: (i.K[k][1], i.K[k][0]))
            if first != tied[0]:
                return True
    return False


def _boundary(i):
    xs = {k[0] for k in i.K}
    return any({b - 1, b, b + 1} <= xs for b in (OD.column_box(c, i.hX)[0] for c in range(1, i.n_ini)))


def _same_bin(i):
    for sweep in i.deep_sweeps():
        deeper = [p for p in sweep if len(p) - 1 > i.D0]
        heads = [p[:i.D0 + 1] for p in deeper]
        if len(heads) != len(set(heads)):
            return True
    return False


def _tight(i):
    """64 dots inside 32 x 32 px, and the list ends with N + 2 nodes."""
    xs, ys = [k[0] for k in i.K], [k[1] for k in i.K]
    return len(i.K) == 64 and max(max(xs) - min(xs), max(ys) - min(ys)) < 32 and len(i.kept) == i.N + 2


# groups A - C: one predicate per class, wanted in both forms
FORM_CLASSES = {
    "A reach N exactly": lambda i: i.tr.full_end == "reached N" and i.tr.full_passes >= 2 and i.tr.pass_lengths[-1] == i.N,
    "A reach N, over": lambda i: i.tr.full_end == "reached N" and i.tr.pass_lengths[-1] > i.N,
    "A no growth, K = 1": lambda i: i.tr.full_end == "no growth" and len(i.K) == 1,
    "A no growth, K = 2": lambda i: i.tr.full_end == "no growth" and len(i.K) == 2 and len(i.kept) == 2,
    "A no growth, one column": lambda i: (i.tr.full_end == "no growth" and len(i.K) > 2 and len(i.kept) == len(i.K)
                                          and len(i.columns) == 1 and i.n_ini > 1),
    "A switch == N, first pass": lambda i: _switch(i, 0, True),
    "A switch == N + 1, first pass": lambda i: _switch(i, 1, True),
    "A switch == N, later pass": lambda i: _switch(i, 0, False),
    "A switch == N + 1, later pass": lambda i: _switch(i, 1, False),
    "A below D0, reach N": lambda i: i.tr.full_passes > i.D0 and i.tr.full_end == "reached N",
    "A below D0, no growth": lambda i: i.tr.full_passes > i.D0 and i.tr.full_end == "no growth",
    "A below D0, careful": lambda i: i.tr.full_passes > i.D0 and i.tr.full_end == "careful",
    "B break at N": lambda i: _broke(i) and _last(i).length == i.N,
    "B break at N + 1": lambda i: _broke(i) and _last(i).length == i.N + 1,
    "B break at N + 2": lambda i: _broke(i) and _last(i).length == i.N + 2,
    "B growth 0 before the break": lambda i: _broke(i) and any(c[3] == 1 for c in _last(i).candidates[:_last(i).divided - 1]),
    "B 2 children at the break": lambda i: _broke(i) and _last(i).candidates[_last(i).divided - 1][3] == 2,
    "B 3 children at the break": lambda i: _broke(i) and _last(i).candidates[_last(i).divided - 1][3] == 3,
    "B 4 children at the break": lambda i: _broke(i) and _last(i).candidates[_last(i).divided - 1][3] == 4,
    "B break at the first candidate": lambda i: _broke(i) and _last(i).divided == 1 and len(_last(i).candidates) >= 2,
    "B break at the last candidate": lambda i: (_broke(i) and _last(i).divided == len(_last(i).candidates)
                                                and len(_last(i).candidates) >= 2),
    "B 1 iteration": lambda i: len(i.tr.careful) == 1,
    "B 2 iterations": lambda i: len(i.tr.careful) == 2,
    "B 3 or more iterations": lambda i: len(i.tr.careful) >= 3,
    "B ends without growth": lambda i: i.tr.careful_end == "no growth",
    "B tie of 2 straddles": lambda i: _run(i, lambda r: r[3] and r[2] == 2) and sorted(i.kept) != sorted(i.kept_reversed),
    "B tie of 4 or more straddles": lambda i: _run(i, lambda r: r[3] and r[2] >= 4) and sorted(i.kept) != sorted(i.kept_reversed),
    "B tie wholly before the break": lambda i: (_run(i, lambda r: r[1] + r[2] == _last(i).divided)
                                                and not any(r[3] for it in i.tr.careful for r in it.runs)
                                                and sorted(i.kept) == sorted(i.kept_reversed)),
    "B tie deeper than D0 straddles": lambda i: (_run(i, lambda r: r[3] and all(
        c[2] > i.D0 for c in _last(i).candidates[r[1]:r[1] + r[2]])) and sorted(i.kept) != sorted(i.kept_reversed)),
    "B largest candidate 15": lambda i: _max_size(i, 15),
    "B largest candidate 16": lambda i: _max_size(i, 16),
    "B largest candidate 255": lambda i: _max_size(i, 255),
    "B largest candidate 256": lambda i: _max_size(i, 256),
    "B M = 1": lambda i: _M(i, 1),
    "B M = 7": lambda i: _M(i, 7),
    "B M = 8": lambda i: _M(i, 8),
    "B M = 9": lambda i: _M(i, 9),
    "B M = 63": lambda i: _M(i, 63),
    "B M = 64": lambda i: _M(i, 64),
    "B M = 65": lambda i: _M(i, 65),
    "B M > 256": lambda i: any(len(it.candidates) > 256 for it in i.tr.careful),
    "C divided at D0 - 1": lambda i: i.D0 - 1 in i.tr.divided_depths,
    "C divided at D0": lambda i: i.D0 in i.tr.divided_depths,
    "C divided at D0 + 1": lambda i: i.D0 + 1 in i.tr.divided_depths,
    "C divided at D0 + 2": lambda i: i.D0 + 2 in i.tr.divided_depths,
    "C one deep node in a sweep": lambda i: any(len(s) == 1 for s in i.deep_sweeps()),
    "C two deep nodes in a sweep": lambda i: any(len(s) == 2 for s in i.deep_sweeps()),
    "C many deep nodes in a sweep": lambda i: any(len(s) >= 8 for s in i.deep_sweeps()),
    "C two deep nodes in one bin": _same_bin,
    "C final node deeper than D0": lambda i: any(f[0] > i.D0 for f in i.tr.final),
}

# [lds] needs N >= 507, i.e. a list of some 500 nodes at the decision, and D0 = 5 at 400 x 200: a node of depth 5
# is 6 x 6 px and holds at most 4 dots, one of depth 6 is 3 x 3 px and holds one
_SMALL = "a node deeper than D0 = 5 is at most 3 x 3 px and cannot hold two dots 4 px apart"
LDS_OUT_OF_REACH = {
    "A reach N, over": "after the first pass S_j <= S_(j-1) + 3 nexp_(j-1) <= N: only the first pass, of at most 4 nIni "
                       "nodes, can pass N",
    "A switch == N, first pass": "S + 3 nexp <= 16 nIni after the first pass",
    "A switch == N + 1, first pass": "S + 3 nexp <= 16 nIni after the first pass",
    "A below D0, careful": _SMALL,
    "B tie deeper than D0 straddles": _SMALL,
    "B largest candidate 255": "a careful phase at N >= 507 starts at depth >= 3, whose nodes hold at most 132 dots",
    "B largest candidate 256": "a careful phase at N >= 507 starts at depth >= 3, whose nodes hold at most 132 dots",
    "C divided at D0 + 1": _SMALL,
    "C divided at D0 + 2": _SMALL,
    "C two deep nodes in one bin": _SMALL,
}

PLAIN_CLASSES = {
    "A N within the initial columns": lambda i: (i.N <= len(i.columns) and i.N + 2 < 4 * i.n_ini
                                                 and i.tr.full_passes == 1 and len(i.kept) > i.N),
    "C tight cluster, N = 20, ends at N + 2": lambda i: i.N == 20 and _tight(i),
    "C tight cluster, N = 40, ends at N + 2": lambda i: i.N == 40 and _tight(i),
    "D nIni = 1": lambda i: i.n_ini == 1 and len(i.K) > 1,
    "D nIni = 2": lambda i: i.n_ini == 2 and len(i.columns) == 2,
    "D nIni = 3": lambda i: i.n_ini == 3 and len(i.columns) == 3,
    "D empty first column": lambda i: i.n_ini == 3 and i.columns == [1, 2],
    "D empty middle column": lambda i: i.n_ini == 3 and i.columns == [0, 2],
    "D empty last column": lambda i: i.n_ini == 3 and i.columns == [0, 1],
    "D dots on and beside a column boundary": _boundary,
    "D dots at mx, mx - 1, my, my - 1 of odd boxes": lambda i: _split_edges(i, 1),
    "D dots at mx, mx - 1, my, my - 1 of even boxes": lambda i: _split_edges(i, 0),
    "D extreme positions": lambda i: ({3, i.sx - 4} <= {k[0] for k in i.K} and {3, i.sy - 4} <= {k[1] for k in i.K}),
    "E equal maxima, key order against raster order": _raster_disagrees,
    "E unique maximum at the first key": lambda i: any(f[1] >= 3 and f[2] == [f[3]] for f in i.tr.final),
    "E unique maximum at the last key": lambda i: any(f[1] >= 3 and f[2] == [f[4]] for f in i.tr.final),
    "E kept response >= 128": lambda i: any(k[2] >= 128 for k in i.kept),
    "E kept response 20": lambda i: any(k[2] == 20 for k in i.kept),
    "E kept response 154": lambda i: any(k[2] == 154 for k in i.kept),
    "E kept response 254": lambda i: any(k[2] == 254 for k in i.kept),
    "F kp_cap 512": lambda i: i.max_ncap == 512 and len(i.K) > 3000,
    "F kp_cap 513": lambda i: i.max_ncap == 513 and len(i.K) > 3000,
    "F more keys than the cell table": lambda i: len(i.K) > key_table_cap(i.max_ncap),
    "F the same dots thinned below it": lambda i: 2000 < len(i.K) <= key_table_cap(i.max_ncap) < 3000,
    "G level 1, careful phase": lambda i: i.case.level == 1 and _broke(i),
    "G level 1, below the bins": lambda i: i.case.level == 1 and any(d >= i.D0 for d in i.tr.divided_depths),
}


def _formed(name, form, pred):
    return lambda i: i.form == form and pred(i)


CLASSES = dict(PLAIN_CLASSES)
for _name, _pred in FORM_CLASSES.items():
    CLASSES[f"{_name} [flat]"] = _formed(_name, "flat", _pred)
    if _name not in LDS_OUT_OF_REACH:
        CLASSES[f"{_name} [lds]"] = _formed(_name, "lds", _pred)


@functools.lru_cache(maxsize=None)
def ref(case: Case) -> tuple:
    """The oracle's keypoints and descriptors of the case's image."""
    return O.OracleExtractor(**case.params).extract(image(case))


def reached(case: Case) -> list:
    """Every class of CLASSES the case reaches, claimed or not."""
    return [n for n, p in CLASSES.items() if p(info(case))]


# ---- the set ---------------------------------------------------------------------------------------------------------
# Seeds, quotas and N were searched for with the predicates above (a stream of recipes, N taken from each image's
# own pass table: S_j, S_j + 3 nexp_j and their neighbours); a case claims the classes it was chosen for and may
# reach more (reached()).
_SPREAD = tuple(range(0, 200, 7))     # a count per node drawn from 0, 7, ..., 196

CASES: tuple = (
    Case('A N within the initial columns', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 1,
         ('A N within the initial columns',
          'A reach N, over [flat]',
          'C divided at D0 - 1 [flat]',
          'D nIni = 2',
          'E kept response >= 128',
          'F more keys than the cell table',)),
    Case('A below D0, careful, flat', 'big', 'clusters', (633247, 1, 6, 18, 8), 15,
         ('A below D0, careful [flat]',)),
    Case('A below D0, no growth, flat', 'big', 'sprinkle', (90345, 3, (0, 1, 2, 2, 3, 3)), 363,
         ('A below D0, no growth [flat]',)),
    Case('A below D0, no growth, lds', 'big', 'sprinkle', (81389, 5, (0, 0, 0, 1), ((6, 4, 4),)), 777,
         ('A below D0, no growth [lds]',
          'A switch == N, later pass [lds]',)),
    Case('A below D0, reach N, lds', 'big', 'full_quads', (2, 4, 400, 20), 540,
         ('A below D0, reach N [lds]',)),
    Case('A below D0, reach N, flat', 'four', 'clusters', (560829, 1, 5, 10, 3), 7,
         ('A below D0, reach N [flat]',)),
    Case('A no growth, K = 1, flat', 'two', 'mixed', (0, ((19, 52, 127),), 0), 2,
         ('A no growth, K = 1 [flat]',)),
    Case('A no growth, K = 1, lds', 'big', 'scatter', (77434, 1), 577,
         ('A no growth, K = 1 [lds]',)),
    Case('A no growth, K = 2, flat', 'three', 'mixed', (0, ((70, 49, 251), (43, 50, 139)), 0), 3,
         ('A no growth, K = 2 [flat]',)),
    Case('A no growth, K = 2, lds', 'big', 'scatter', (22811, 2), 715,
         ('A no growth, K = 2 [lds]',)),
    Case('A no growth, one column, flat', 'big', 'mixed', (0, ((43, 50, 173), (164, 36, 209), (46, 160, 136)), 0), 4,
         ('A no growth, one column [flat]',)),
    Case('A one column', 'big', 'scatter', (3, 5, (19, 19, 150, 180)), 600,
         ('A no growth, one column [lds]',)),
    Case('A reach N exactly, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 124,
         ('A reach N exactly [flat]',
          'A switch == N, later pass [flat]',)),
    Case('A reach N exactly, lds', 'big', 'sprinkle', (54369, 4, (1,), ((0, 0, 0), (64, 2, 4))), 512,
         ('A reach N exactly [lds]',)),
    Case('A switch == N + 1, first pass, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 31,
         ('A switch == N + 1, first pass [flat]',)),
    Case('A switch == N + 1, first pass, flat (twin)', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 31,
         ('A switch == N + 1, first pass [flat]',)),
    Case('A switch == N + 1, later pass, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 123,
         ('A switch == N + 1, later pass [flat]',)),
    Case('A switch == N + 1, later pass, flat (twin)', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 123,
         ('A switch == N + 1, later pass [flat]',)),
    Case('A switch == N + 1, later pass, lds', 'big', 'sprinkle', (81389, 5, (0, 0, 0, 1), ((6, 4, 4),)), 776,
         ('A switch == N + 1, later pass [lds]',)),
    Case('A switch == N + 1, later pass, lds (twin)', 'big', 'sprinkle', (81389, 5, (0, 0, 0, 1), ((6, 4, 4),)), 776,
         ('A switch == N + 1, later pass [lds]',)),
    Case('A switch == N, first pass, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 32,
         ('A switch == N, first pass [flat]',)),
    Case('B 1 iteration, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 9,
         ('B 1 iteration [flat]',
          'B 4 children at the break [flat]',
          'B M = 8 [flat]',
          'B break at N + 2 [flat]',
          'B break at the first candidate [flat]',)),
    Case('B 1 iteration, lds', 'big', 'sprinkle', (14178, 4, (1, 2), ((24, 0, 0), (23, 3, 8))), 512,
         ('B 1 iteration [lds]',)),
    Case('B 2 children at the break, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 468,
         ('B 2 children at the break [flat]',)),
    Case('B 2 children at the break, lds', 'big', 'sprinkle', (81389, 5, (0, 0, 0, 1), ((6, 4, 4),)), 509,
         ('B 2 children at the break [lds]',
          'B 2 iterations [lds]',
          'B break at N [lds]',
          'B tie of 4 or more straddles [lds]',
          'C divided at D0 - 1 [lds]',
          'C divided at D0 [lds]',
          'C final node deeper than D0 [lds]',)),
    Case('B 2 iterations, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 470,
         ('B 2 iterations [flat]',
          'B M > 256 [flat]',)),
    Case('B 3 children at the break, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 24,
         ('B 3 children at the break [flat]',
          'F the same dots thinned below it',)),
    Case('B 3 children at the break, lds', 'big', 'sprinkle', (63828, 4, (0, 1, 1, 1, 2, 3)), 509,
         ('B 3 children at the break [lds]',)),
    Case('B 3 or more iterations, flat', 'big', 'sprinkle', (90345, 3, (0, 1, 2, 2, 3, 3)), 221,
         ('B 3 or more iterations [flat]',
          'B M = 9 [flat]',
          'C divided at D0 [flat]',
          'C final node deeper than D0 [flat]',
          'C many deep nodes in a sweep [flat]',)),
    Case('B 3 or more iterations, lds', 'big', 'sprinkle', (81389, 5, (0, 0, 0, 1), ((6, 4, 4),)), 511,
         ('B 3 or more iterations [lds]',
          'B ends without growth [lds]',)),
    Case('B 4 children at the break, lds', 'big', 'sprinkle', (14178, 4, (1, 2), ((24, 0, 0), (23, 3, 8))), 510,
         ('B 4 children at the break [lds]',
          'B break at N + 2 [lds]',)),
    Case('B M = 1, flat', 'four', 'clusters', (67268, 1, 2, 6, 1), 3,
         ('B M = 1 [flat]',)),
    Case('B M = 1, lds', 'big', 'sprinkle', (97970, 4, (1,), ((2, 0, 0), (1, 2, 4))), 511,
         ('B M = 1 [lds]',)),
    Case('B M = 63, flat', 'big', 'sprinkle', (23413, 3, (0, 1), ((63, 2, 5),)), 101,
         ('B M = 63 [flat]',)),
    Case('B M = 63, lds', 'big', 'sprinkle', (43819, 4, (1,), ((2, 0, 0), (63, 2, 4))), 511,
         ('B M = 63 [lds]',)),
    Case('B M = 64, flat', 'big', 'sprinkle', (6553, 3, (0, 1), ((64, 2, 5),)), 95,
         ('B M = 64 [flat]',)),
    Case('B M = 64, lds', 'big', 'sprinkle', (54369, 4, (1,), ((0, 0, 0), (64, 2, 4))), 513,
         ('B M = 64 [lds]',)),
    Case('B M = 65, flat', 'big', 'sprinkle', (99350, 3, (0, 1), ((65, 2, 5),)), 96,
         ('B M = 65 [flat]',)),
    Case('B M = 65, lds', 'big', 'sprinkle', (19729, 4, (1,), ((0, 0, 0), (65, 2, 4))), 513,
         ('B M = 65 [lds]',)),
    Case('B M = 7, flat', 'two', 'scatter', (75135, 20, None, 121, 121), 9,
         ('B M = 7 [flat]',)),
    Case('B M = 7, lds', 'big', 'sprinkle', (51912, 5, (0, 0, 0, 1), ((11, 4, 4),)), 509,
         ('B M = 7 [lds]',)),
    Case('B M = 8, lds', 'big', 'sprinkle', (30530, 5, (0, 0, 0, 1), ((19, 4, 4),)), 565,
         ('B M = 8 [lds]',)),
    Case('B M = 9, lds', 'big', 'sprinkle', (48839, 5, (0, 1, 1, 1), ((19, 2, 4),)), 1543,
         ('B M = 9 [lds]',)),
    Case('B M > 256, lds', 'big', 'sprinkle', (64199, 4, (1, 2), ((8, 0, 0), (20, 3, 8))), 510,
         ('B M > 256 [lds]',)),
    Case('B break at N + 1, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 10,
         ('B break at N + 1 [flat]',)),
    Case('B break at N + 1, lds', 'big', 'sprinkle', (14178, 4, (1, 2), ((24, 0, 0), (23, 3, 8))), 511,
         ('B break at N + 1 [lds]',)),
    Case('B break at N, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 11,
         ('B break at N [flat]',)),
    Case('B break at the first candidate, lds', 'big', 'sprinkle', (14178, 4, (1, 2), ((24, 0, 0), (23, 3, 8))), 744,
         ('B break at the first candidate [lds]',
          'C many deep nodes in a sweep [lds]',)),
    Case('B break at the last candidate, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 30,
         ('B break at the last candidate [flat]',)),
    Case('B break at the last candidate, lds', 'big', 'sprinkle', (81389, 5, (0, 0, 0, 1), ((6, 4, 4),)), 510,
         ('B break at the last candidate [lds]',
          'B tie wholly before the break [lds]',)),
    Case('B ends without growth, flat', 'big', 'sprinkle', (90345, 3, (0, 1, 2, 2, 3, 3)), 231,
         ('B ends without growth [flat]',)),
    Case('B growth 0 before the break, flat', 'big', 'sprinkle', (73392, 4, (0, 1, 2, 2, 3, 3)), 426,
         ('B growth 0 before the break [flat]',)),
    Case('B growth 0 before the break, lds', 'big', 'sprinkle', (14178, 4, (1, 2), ((24, 0, 0), (23, 3, 8))), 725,
         ('B growth 0 before the break [lds]',)),
    Case('B largest 255', 'big', 'quota', (3, 1, (255, 100, 90, 80, 70, 60, 50, 40)), 12,
         ('B largest candidate 255 [flat]',)),
    Case('B largest 256', 'big', 'quota', (3, 1, (256, 100, 90, 80, 70, 60, 50, 40)), 12,
         ('B largest candidate 256 [flat]',)),
    Case('B largest candidate 15, flat', 'big', 'sprinkle', (99350, 3, (0, 1), ((65, 2, 5),)), 33,
         ('B largest candidate 15 [flat]',)),
    Case('B largest candidate 15, lds', 'big', 'sprinkle', (28101, 4, (1, 2), ((21, 0, 0), (35, 3, 8))), 510,
         ('B largest candidate 15 [lds]',)),
    Case('B largest candidate 16, flat', 'three', 'patch', (17632, 180, 32, 8, 8, 0), 10,
         ('B largest candidate 16 [flat]',)),
    Case('B largest candidate 16, lds', 'big', 'sprinkle', (53646, 5, (0, 1, 1, 1), ((5, 2, 4),)), 509,
         ('B largest candidate 16 [lds]',)),
    Case('B largest candidate 256, flat', 'big', 'quota', (85287, 3, (), 16), 9,
         ('B largest candidate 256 [flat]',)),
    Case('B tie deeper than D0 straddles, flat', 'big', 'clusters', (35463, 5, 3, 9, 6), 15,
         ('B tie deeper than D0 straddles [flat]',
          'C divided at D0 + 1 [flat]',)),
    Case('B tie of 2 straddles, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 93,
         ('B tie of 2 straddles [flat]',)),
    Case('B tie of 2 straddles, lds', 'big', 'sprinkle', (20136, 5, (0, 0, 0, 1), ((16, 4, 4),)), 529,
         ('B tie of 2 straddles [lds]',)),
    Case('B tie of 4 or more straddles, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 62,
         ('B tie of 4 or more straddles [flat]',
          'E unique maximum at the last key',)),
    Case('B tie wholly before the break, flat', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255, 255),)), 40,
         ('B tie wholly before the break [flat]',
          'E unique maximum at the first key',)),
    Case('C divided at D0 + 2, flat', 'big', 'clusters', (203767, 1, 6, 22, 3), 9,
         ('C divided at D0 + 2 [flat]',)),
    Case('C one deep node in a sweep, flat', 'three', 'mixed', (58226, ((84, 30, 150), (85, 34, 160), (86, 38,
         170), (19, 19, 140), (220, 19, 150), (19, 80, 160), (220, 80, 170)), 100), 107,
         ('C one deep node in a sweep [flat]',)),
    Case('C one deep node in a sweep, lds', 'big', 'sprinkle', (53646, 5, (0, 1, 1, 1), ((5, 2, 4),)), 1533,
         ('C one deep node in a sweep [lds]',)),
    Case('C tight cluster, N = 20', 'sq', 'patch', (1, 25, 37, 8, 8, 0), 20,
         ('C tight cluster, N = 20, ends at N + 2',)),
    Case('C tight cluster, N = 40', 'sq', 'patch', (1, 19, 37, 8, 8, 0), 40,
         ('C tight cluster, N = 40, ends at N + 2',)),
    Case('C two deep nodes in a sweep, flat', 'big', 'scatter', (38141, 150, None, 121, 121), 149,
         ('C two deep nodes in a sweep [flat]',)),
    Case('C two deep nodes in a sweep, lds', 'big', 'sprinkle', (51743, 5, (0, 1, 1, 1), ((4, 2, 4),)), 1556,
         ('C two deep nodes in a sweep [lds]',)),
    Case('C two deep nodes in one bin, flat', 'big', 'clusters', (633247, 1, 6, 18, 8), 13,
         ('C two deep nodes in one bin [flat]',)),
    Case('D dots at mx, mx - 1, my, my - 1 of even boxes', 'big', 'scatter', (86670, 200), 1,
         ('D dots at mx, mx - 1, my, my - 1 of even boxes',)),
    Case('D dots at mx, mx - 1, my, my - 1 of odd boxes', 'three', 'mixed', (58226, ((84, 30, 150), (85, 34,
         160), (86, 38, 170), (19, 19, 140), (220, 19, 150), (19, 80, 160), (220, 80, 170)), 100), 88,
         ('D dots at mx, mx - 1, my, my - 1 of odd boxes',)),
    Case('D dots on and beside a column boundary', 'three', 'mixed', (58226, ((84, 30, 150), (85, 34, 160), (86,
         38, 170), (19, 19, 140), (220, 19, 150), (19, 80, 160), (220, 80, 170)), 100), 1,
         ('D dots on and beside a column boundary',
          'D extreme positions',)),
    Case('D empty first column', 'three', 'patch', (86302, 147, 39, 8, 8, 0), 1,
         ('D empty first column',)),
    Case('D empty last column', 'three', 'clusters', (68408, 2, 7, 20, 2), 1,
         ('D empty last column',)),
    Case('D empty middle column', 'three', 'mixed', (0, ((24, 29, 137), (65, 74, 155), (64, 39, 127), (209, 64,
         230)), 0), 1,
         ('D empty middle column',)),
    Case('D nIni = 1', 'sq', 'patch', (11488, 62, 23, 8, 8, 0), 1,
         ('D nIni = 1',)),
    Case('D nIni = 3', 'three', 'clusters', (24926, 2, 8, 16, 10), 1,
         ('D nIni = 3',)),
    Case('E equal maxima, key order against raster order', 'big', 'sprinkle', (69921, 2, _SPREAD, ((1, 255,
         255),)), 12,
         ('E equal maxima, key order against raster order',)),
    Case('E kept response 154', 'sq', 'scatter', (732433, 20, None, 255, 255), 1,
         ('E kept response 154',)),
    Case('E kept response 20', 'big', 'sprinkle', (46519, 4, (0, 1, 2, 2, 3, 3)), 254,
         ('E kept response 20',)),
    Case('E response 254', 'sq', 'scatter', (5, 30, None, 250, 255), 10,
         ('E kept response 254',), 0, 0),
    Case('F key table', 'big', 'quota', (1, 0, (1100, 1100)), 12,
         ('F the same dots thinned below it',)),
    Case('F key walk', 'big', 'quota', (1, 0, ()), 12,
         ('F more keys than the cell table',)),
    Case('F nfeatures 508', 'big', 'quota', (1, 0, ()), 508,
         ('F kp_cap 512',)),
    Case('F nfeatures 509', 'big', 'quota', (1, 0, ()), 509,
         ('F kp_cap 513',)),
    Case('G level 1, below the bins', 'two', 'clusters', (757, 2, 5, 16, 4), 44,
         ('G level 1, below the bins',), 100, 1),
    Case('G level 1, careful phase', 'odd', 'clusters', (828, 2, 2, 16, 23), 48,
         ('G level 1, careful phase',), 100, 1),
)


def by_name(name: str) -> Case:
    return next(c for c in CASES if c.name == name)
