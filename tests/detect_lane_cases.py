"""Small single-level images that put one FAST cell of k_detect's two-queue path (minTh < iniTh) on each side of
the decisions its lanes take: which B entries the idle lanes of A's last M step carry, and whether a pre-test half
(64 quads; two per iteration, the last iteration's second one possibly without a live row) has an A pair.

A = the pixel pairs whose cardinal bound exceeds iniTh, B = those above minTh (A is a subset of B); a cell falls
back to minTh when no iniTh corner survives its NMS.  The images are a flat background with
  dot   an isolated pixel: + 8 .. 20 is a minTh-only corner (one B pair), above + 20 an iniTh corner (one A pair);
  star  a + 30 pixel whose four diagonal circle points are + 15: its bound is 30 but every arc of 9 holds two of
        the + 15 points, so M = 15: one A pair that is no iniTh corner (and five B pairs);
  diag  a 1 px diagonal line from image border to image border: its pixels and the pixels 3 px beside it pass the
        bound with M = 0 (about three A or B pairs per row, no corner);
  fill  n further + 10 dots on a 4 px lattice, clear of the other primitives (n more B pairs).
Coordinates are relative to the target cell's detection window.  tests/test_detect_lane_cases_cpu.py shows with the
numpy restatement (tools/detect_queue_stats.py) and the oracle that every case has the window, the queue lengths
and the outcome it states; tests/test_gpu_detect_lanes.py runs the same images through the kernel."""
import functools
import importlib.util
from pathlib import Path
from typing import NamedTuple

import numpy as np

from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
BG = 100
INI, MIN = 20, 7
PARAMS = dict(nfeatures=500, scaleFactor=1.2, nlevels=1, iniThFAST=INI, minThFAST=MIN)


@functools.lru_cache(maxsize=None)
def model():
    spec = importlib.util.spec_from_file_location("detect_queue_stats", ROOT / "tools" / "detect_queue_stats.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Case(NamedTuple):
    name: str
    size: tuple      # (w, h)
    cell: int        # the target cell, in the reference's cell order
    prims: tuple
    expect: dict     # of the target cell: keys of lane_counts
    classes: tuple

    def __hash__(self):   # the name is unique (the dict is not hashable)
        return hash(self.name)


def grid(size):
    return list(model().cells(*size))


def draw(size, cell, prims):
    w, h = size
    x0, y0, x1, y1 = grid(size)[cell]
    tx, ty, ww, wh = x0 + 3, y0 + 3, x1 - x0 - 6, y1 - y0 - 6
    img = np.full((h, w), BG, np.uint8)
    for p in prims:
        if p[0] == "dot":
            _, x, y, v = p
            img[ty + y, tx + x] = BG + v
        elif p[0] == "star":
            _, x, y = p
            img[ty + y, tx + x] = BG + 30
            for dx in (-2, 2):
                for dy in (-2, 2):
                    img[ty + y + dy, tx + x + dx] = BG + 15
        elif p[0] == "diag":
            _, off, d, v = p
            for Y in range(h):
                X = tx + off + d * (Y - ty)
                if 0 <= X < w:
                    img[Y, X] = BG + v
        elif p[0] == "fill":
            n = p[1]
            busy = np.pad(img != BG, 5)
            for y in range(1, wh - 1, 2):
                for x in range(1 + (y % 4), ww - 1, 4):
                    if n and not busy[ty + y:ty + y + 11, tx + x:tx + x + 11].any():
                        img[ty + y, tx + x] = BG + 10
                        n -= 1
            assert n == 0, f"fill: {n} dots left without a free spot"
        else:
            raise ValueError(p)
    return img


@functools.lru_cache(maxsize=None)
def image(case: Case) -> np.ndarray:
    img = draw(case.size, case.cell, case.prims)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def counts(case: Case) -> tuple:
    """lane_counts of every cell of the case's image, in cell order."""
    D = model()
    M, bound = D.maps(image(case))
    cs = grid(case.size)
    cap = max(D.pair_cap(c) for c in cs)
    return tuple(D.lane_counts(M, bound, c, cap, INI, MIN) for c in cs)


def expected_counters(case: Case) -> list:
    """orbfe_debug_detect_lanes' seven words for one image of the case."""
    cs = counts(case)
    return [len(cs), sum(c["collide"] for c in cs), sum(c["fallback"] for c in cs),
            sum(c["carry_steps"] for c in cs), sum(c["kb"] for c in cs), sum(c["b_steps"] for c in cs),
            sum(c["a_skipped"] for c in cs)]


def model_candidates(case: Case) -> list:
    """The level's candidates by the restatement, as orbfe_debug_candidates / oracle.level_candidates list them:
    cell by cell, a cell's corners row-major, (x, y) relative to the 16 px border, score = M - 1; the iniTh corners
    of a cell, or its minTh corners when it has none."""
    M, _ = model().maps(image(case))
    rows = []
    for x0, y0, x1, y1 in grid(case.size):
        ww, wh = x1 - x0 - 6, y1 - y0 - 6
        Mw = M[y0 + 3:y0 + 3 + wh, x0 + 3:x0 + 3 + ww]
        Z = np.pad(Mw, 1)
        nb = np.max([Z[1 + dy:1 + dy + wh, 1 + dx:1 + dx + ww] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx],
                    axis=0)
        for th in (INI, MIN):
            ys, xs = np.nonzero((Mw > th) & (Mw > nb))
            if len(ys):
                rows += [(int(x0 + 3 + x - 16), int(y0 + 3 + y - 16), int(Mw[y, x] - 1)) for y, x in zip(ys, xs)]
                break
    return rows


@functools.lru_cache(maxsize=None)
def ref(case: Case) -> tuple:
    """The oracle's keypoints and descriptors of the case's image."""
    return O.OracleExtractor(**PARAMS).extract(image(case))


@functools.lru_cache(maxsize=None)
def candidates(case: Case) -> np.ndarray:
    return O.level_candidates(O.OracleExtractor(**PARAMS).p, image(case))


STAR = ("star", 10, 4)
G24, G25, G40, G41, G44 = (95, 62), (95, 63), (95, 78), (95, 79), (95, 82)   # one cell row: wh = h - 38
# 18 cell rows, 17 of 31 window rows and a last one of 8 / 9 (a last row this low needs 18 of them), and wide enough
# for the octree's initial nodes (round(span x / span y) >= 1)
G8, G9 = (304, 573), (304, 574)
W35, W40 = (100, 73), (100, 78)      # 34 px windows: 9 quads per row, the generic pre-test

CASES = (
    # ---- the second half of the last pre-test iteration without a live row (wh - y0 <= 8 at y0 = 0, 16, 32), and
    #      with one
    Case("wh 8", G8, 153, (("star", 10, 4), ("dot", 20, 6, 10)), dict(wh=8, qrow=8, halves=1, halves_empty=1, A=1),
         ("empty half at y0 = 0",)),
    Case("wh 9", G9, 153, (("star", 10, 5), ("dot", 20, 8, 10)), dict(wh=9, qrow=8, halves=2, halves_empty=0, A=1),
         ("live half at y0 = 0",)),
    Case("wh 24", G24, 0, (("star", 10, 20), ("dot", 20, 23, 10)), dict(wh=24, halves=3, halves_empty=1, A=1),
         ("empty half at y0 = 16",)),
    Case("wh 25", G25, 0, (("star", 10, 21), ("dot", 20, 24, 10)), dict(wh=25, halves=4, halves_empty=0, A=1),
         ("live half at y0 = 16",)),
    Case("wh 40", G40, 0, (("star", 10, 36), ("dot", 20, 39, 10)), dict(wh=40, halves=5, halves_empty=1, A=1),
         ("empty half at y0 = 32",)),
    Case("wh 41", G41, 0, (("star", 10, 37), ("dot", 20, 40, 10)), dict(wh=41, halves=6, halves_empty=0, A=1),
         ("live half at y0 = 32",)),
    Case("wh 44, 16 row slots", G44, 0, (("star", 10, 40), ("dot", 20, 43, 30)),
         dict(wh=44, halves=6, halves_empty=0, fallback=False), ("ROI above 48 rows",)),
    Case("9 quads per row, odd halves", W35, 0, (STAR, ("diag", -12, 1, 28), ("fill", 20)),
         dict(wh=35, qrow=9, halves=5, halves_empty=1, fallback=True), ("generic pre-test, empty half",)),
    Case("9 quads per row, even halves", W40, 0, (STAR, ("diag", -12, 1, 28), ("fill", 20)),
         dict(wh=40, qrow=9, halves=6, halves_empty=0, fallback=True), ("generic pre-test, live half",)),
    # ---- the carry: |A| mod 64 and |B| against the free lanes
    Case("A 1, B 5", G40, 0, (STAR,), dict(A=1, B=5, fallback=True, kb=5, b_steps=0, a_halves=[1, 0, 0, 0, 0]),
         ("|A| mod 64 = 1", "|B| < free lanes", "A in the first half")),
    Case("A 1, B 63", G40, 0, (STAR, ("fill", 58)), dict(A=1, B=63, fallback=True, kb=63, b_steps=0), ("|B| = free lanes",)),
    Case("A 1, B 64", G40, 0, (STAR, ("fill", 59)), dict(A=1, B=64, fallback=True, kb=63, b_steps=1),
         ("|B| = free lanes + 1",)),
    Case("A 1, B 127", G40, 0, (STAR, ("diag", 20, -1, 12), ("fill", 59)), dict(A=1, B=127, fallback=True, kb=63, b_steps=1),
         ("|B| - free lanes = 64",)),
    Case("A 63", G40, 0, (("diag", -20, 1, 28), ("star", 24, 6), ("star", 24, 14), ("star", 10, 6)),
         dict(A=63, B=75, fallback=True, kb=1, b_steps=2), ("|A| mod 64 = 63",)),
    Case("A 64", G40, 0, (("diag", -19, 1, 28), ("star", 24, 6)), dict(A=64, B=68, fallback=True, kb=0, carry_steps=0, b_steps=2),
         ("|A| mod 64 = 0",)),
    Case("A 70", G40, 0, (("diag", -17, 1, 28), ("star", 24, 6), ("fill", 10)),
         dict(A=70, B=84, fallback=True, kb=58, b_steps=1), ("|A| > 64",)),
    Case("iniTh corner, B carried", G40, 0, (("dot", 10, 20, 40), ("fill", 30)),
         dict(A=1, B=31, fallback=False, kb=31, b_steps=0), ("no fallback, carried",)),
    Case("second half only", G40, 0, (("star", 10, 11), ("fill", 12)), dict(A=1, B=17, fallback=True, a_halves=[0, 1, 0, 0, 0]),
         ("A in the second half",)),
    # ---- odd width: the window's last pair, whose second pixel lies outside it, among the carried entries; the
    #      outside pixel is the stronger corner, so an uncleared map column would suppress the inside one
    Case("odd width, row end carried", G40, 1, (("star", 10, 20), ("dot", 24, 2, 10), ("dot", 25, 2, 14)),
         dict(ww=25, A=1, B=6, fallback=True, kb=6, b_steps=0), ("row-end pair carried",)),
)

CLASSES = tuple(dict.fromkeys(n for c in CASES for n in c.classes))


def by_name(name):
    return next(c for c in CASES if c.name == name)
