"""Small single-level images that put k_detect's arithmetic on each side of its decisions: the 16 arcs of the exact
M (fast_m_pair), the threshold comparisons and their ends, the eight NMS neighbours and their ties, the detection
window's borders and the one-pass path's fallback copy.  tests/detect_lane_cases.py pins which lanes do what; this
module pins what they compute.

Geometries (nlevels = 1).  k_detect has five instantiations <RP, NS>: RP = the ROI pitch (48 / 64 / 96 for a widest
ROI of at most 45 / 61 / more), NS = 16 for ROIs above 48 rows.  The host refuses a FAST cell ROI wider than 59 px
("FAST cell ROI larger than 59 x 64 px": a ROI row is staged as 16 dwords), and no cell grid yields one (a single
cell column is at most 59 wide, two or more at most 51), so <96, 16> cannot be launched by any accepted geometry
(INSTANTIATION_OUT_OF_REACH): 90 x 70 reaches <64, 12> (ROI 58 wide).  The other four are reached by
  <48, 12>  95 x 62   two cells of 32 / 25 px windows, qrow = 8 / 7: the rows-of-8-lanes pre-test
  <48, 16>  95 x 82   the same, ROI of 50 rows
  <64, 12>  80 x 70   one cell, ROI 48 wide, qrow = 11: the generic pre-test
  <64, 16>  80 x 85   ROI 48 x 53
for family A, and by 2 x 2 cell geometries for the other families (102 x 108, 102 x 118, 116 x 108, 116 x 118;
102 x 108 has its cell boundaries at x = 53 | 54 and y = 56 | 57), with 104 / 106 / 108 x 108 for the window widths
with ww mod 4 = 2, 3, 0 and 117 x 108 / 118 for an odd window width at RP = 64.

Families (background 100, (iniTh, minTh) = (20, 7) unless the case says otherwise):
  A  arcs: a stamp whose centre is a corner through arc k alone (M = 32, response 31), bright and dark, the centre
     first and second pixel of its pair, and the negative (an arc of 8); also run at (20, 20) and (7, 7);
  B  threshold sides: dots of + 7 / 8 / 20 / 21, the fallback, the ends 0 / 1 / 2 / 254 / 255, minTh > iniTh;
  C  NMS: a weaker and a stronger (or equal) dot in each of the 8 directions, the weaker on both pixels of a pair;
  D  windows: pairs across cell boundaries (both kept) and across the level's outer window edges (the outside pixel
     is in no window);
  E  one-pass path (the two queues meet) whose minTh list is copied out, and discarded.

restate() is the numpy restatement (tools/detect_queue_stats.py's maps, cv::FAST's score and strict NMS per cell
window, the iniTh -> minTh fallback) with one mutant per decision; tests/test_detect_fast_cases_cpu.py shows that it
equals the oracle on every case and that every case's candidate list changes under the mutants it is named for;
tests/test_gpu_detect_fast.py runs the same images through the kernel."""
import functools
from typing import NamedTuple

import numpy as np

import detect_lane_cases as L
from oracle import oracle as O

BG = L.BG
model = L.model
grid = L.grid

# ---------------------------------------------------------------------------------------------- geometry
INSTANTIATIONS = ((48, 12), (48, 16), (64, 12), (64, 16), (96, 16))
INSTANTIATION_OUT_OF_REACH = {
    (96, 16): "RP = 96 needs a ROI wider than 61 px; the host refuses ROIs wider than 59 px and no cell grid yields "
              "one (one cell column: at most 59, more: at most 51)",
}
REACHED = tuple(i for i in INSTANTIATIONS if i not in INSTANTIATION_OUT_OF_REACH)
GEO_A = {(48, 12): (95, 62), (48, 16): (95, 82), (64, 12): (80, 70), (64, 16): (80, 85)}
GEO_22 = {(48, 12): (102, 108), (48, 16): (102, 118), (64, 12): (116, 108), (64, 16): (116, 118)}
GEO_WIDTHS = ((102, 108), (104, 108), (106, 108), (108, 108))   # last cell column: ww = 29, 30, 31, 32
GEO_ODD_64 = {(64, 12): (117, 108), (64, 16): (117, 118)}       # first cell column: ww = 43 (116 wide: 42 and 36)


def detect_rp(max_rw):
    return 48 if max_rw + 3 <= 48 else 64 if max_rw + 3 <= 64 else 96


@functools.lru_cache(maxsize=None)
def geometry(size):
    """What the host derives from a level's cell grid: the instantiation, and per cell qrow (quads per window row)
    and rem (pixels of a row's last quad inside the window); accepted = the host takes the ROI sizes."""
    cs = grid(size)
    max_rw, max_rh = max(c[2] - c[0] for c in cs), max(c[3] - c[1] for c in cs)
    rp, tall = detect_rp(max_rw), max_rh > 48
    ww = [c[2] - c[0] - 6 for c in cs]
    qrow = [(w + 3) >> 2 for w in ww]
    return dict(inst=(rp, 16 if tall or rp == 96 else 12), accepted=max_rw <= 59 and max_rh <= 64 and cs[0][0] >= 1,
                qrow=qrow, rem=[w - 4 * (q - 1) for w, q in zip(ww, qrow)], ncells=len(cs))


def window(size, cell):
    """(tx, ty, ww, wh): the cell's detection window in image coordinates."""
    x0, y0, x1, y1 = grid(size)[cell]
    return x0 + 3, y0 + 3, x1 - x0 - 6, y1 - y0 - 6


# ---------------------------------------------------------------------------------------------- restatement
DIRS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
MUTANT_CLASSES = ("arc", "nms_dir", "nms_ge", "th_ge", "window", "nms_across", "fallback_pre", "onepass_never",
                  "onepass_always")


def m_map(img, drop=None):
    """The exact FAST M of every pixel; drop = (k, bright): without arc k of that polarity."""
    D = model()
    if drop is None:
        return D.maps(img)[0]
    I = img.astype(np.int32)
    h, w = I.shape
    P = np.pad(I, 3, mode="edge")
    d = np.stack([I - P[3 + dy:3 + dy + h, 3 + dx:3 + dx + w] for dx, dy in D.CIRCLE])
    M = np.zeros((h, w), np.int32)
    for k in range(16):
        idx = [(k + j) % 16 for j in range(9)]
        if drop != (k, True):
            M = np.maximum(M, d[idx].min(0))       # the centre brighter than the arc
        if drop != (k, False):
            M = np.maximum(M, (-d[idx]).min(0))
    return M


def restate(img, th=(L.INI, L.MIN), mut=None):
    """The level's candidates as oracle.level_candidates lists them (cell by cell, row-major, relative to the 16 px
    border, score = M - 1): cv::FAST with non-maximum suppression on each cell's window at iniTh, and at minTh for a
    cell where that kept nothing.  mut = None, or one decision changed: ("arc", k, bright), ("nms_dir", (dx, dy)),
    ("nms_ge",), ("th_ge",), ("window", side) (one more column / row on side l, r, t or b), ("nms_across",),
    ("fallback_pre",) (fall back when no iniTh corner exists before the NMS), ("onepass_never",) / ("onepass_always",)
    (a cell on the kernel's one-pass path never / always takes its minTh list)."""
    D = model()
    kind = mut[0] if mut else None
    img = np.asarray(img)
    h, w = img.shape
    ini, mn = (min(max(int(t), 0), 255) for t in th)
    M = m_map(img, (mut[1], mut[2]) if kind == "arc" else None)
    cs = grid((w, h))
    cap = max(D.pair_cap(c) for c in cs)
    bound = D.maps(img)[1] if kind in ("onepass_never", "onepass_always") else None
    dirs = [d for d in DIRS if not (kind == "nms_dir" and d == tuple(mut[1]))]
    rows = []
    for cell in cs:
        x0, y0, x1, y1 = cell
        wx0, wy0, wx1, wy1 = x0 + 3, y0 + 3, x1 - 3, y1 - 3
        if kind == "window":
            wx0, wy0 = wx0 - (mut[1] == "l"), wy0 - (mut[1] == "t")
            wx1, wy1 = wx1 + (mut[1] == "r"), wy1 + (mut[1] == "b")
        inside = np.zeros((h, w), bool)
        inside[wy0:wy1, wx0:wx1] = True

        def fast_at(t, pre=False):
            corner = (M >= t if kind == "th_ge" else M > t) & (M > 0)
            if pre:
                return bool((corner & inside).any())
            S = np.where(corner, M - 1, 0)
            Z = np.pad(S if kind == "nms_across" else np.where(inside, S, 0), 1)
            nb = np.max([Z[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dx, dy in dirs], axis=0)
            keep = corner & inside & (S >= nb if kind == "nms_ge" else S > nb)
            ys, xs = np.nonzero(keep)
            return [(int(x - 16), int(y - 16), int(S[y, x])) for y, x in zip(ys, xs)]

        got = fast_at(ini)
        if kind == "fallback_pre":
            if not fast_at(ini, pre=True):
                got = fast_at(mn)
        elif kind in ("onepass_never", "onepass_always") and (
                mn >= ini or D.lane_counts(M, bound, cell, cap, ini, mn)["collide"]):
            if kind == "onepass_always" and mn != ini:
                got = fast_at(mn) or got
        elif not got:
            got = fast_at(mn)
        rows += got
    return rows


# ---------------------------------------------------------------------------------------------- cases
class Case(NamedTuple):
    name: str
    family: str
    size: tuple       # (w, h)
    th: tuple         # (iniTh, minTh)
    img: np.ndarray
    classes: tuple    # what the case is named for (test_detect_fast_cases_cpu.REQUIRED)
    mutants: tuple    # the candidate list changes under each of these
    expect: tuple     # None, or the candidates as a sorted tuple of (x, y, response), image coordinates
    info: dict        # family specific: what the CPU test asserts besides

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self.name == other.name

    @property
    def inst(self):
        return geometry(self.size)["inst"]

    @property
    def params(self):
        return dict(L.PARAMS, iniThFAST=self.th[0], minThFAST=self.th[1])


def _blank(size, v=BG):
    return np.full((size[1], size[0]), v, np.uint8)


def _case(name, family, size, img, classes, mutants, expect=None, th=(L.INI, L.MIN), **info):
    img.setflags(write=False)
    if expect is not None:
        expect = tuple(sorted(expect))
    return Case(name, family, size, th, img, tuple(classes), tuple(mutants), expect, info)


# ---- A. arcs
def stamp(img, cx, cy, k, bright, cut=None):
    """Circle points k .. k + 8 at a +/- j, the other seven at the centre's value: the centre's only arc of 9 is arc
    k, M = 32.  cut = 0 or 8: that end of the arc back at the centre's value (an arc of 8, M = 0)."""
    C = model().CIRCLE
    c, a = (BG + 40, BG) if bright else (BG, BG + 40)
    img[cy, cx] = c
    for dx, dy in C:
        img[cy + dy, cx + dx] = c
    for j in range(9):
        dx, dy = C[(k + j) % 16]
        img[cy + dy, cx + dx] = c if j == cut else (a + j if bright else a - j)


def _slots(size, n):
    """Stamp centres a geometry offers to its image n, (cell, column group, row): groups 10 px apart from the window's
    first column, and one at its last; rows likewise.  A group's column is chosen by the stamp's parity.  Adjacent
    windows tile the level: even images leave out the first group of a cell with a left neighbour, odd ones the last
    group of a cell with a right neighbour."""
    out = []
    cs = grid(size)
    assert len({c[1] for c in cs}) == 1, "one cell row"
    for cell in range(len(cs)):
        tx, ty, ww, wh = window(size, cell)
        last = {p: (ww - 1 if (ww - 1) % 2 == p else ww - 2) for p in (0, 1)}
        groups = [{0: x, 1: x + 1} for x in range(0, ww - 12, 10)] + [last]
        if n % 2 == 0 and cell > 0:
            groups = groups[1:]
        if n % 2 == 1 and cell + 1 < len(cs):
            groups = groups[:-1]
        out += [(cell, g, y) for y in list(range(0, wh - 10, 10)) + [wh - 1] for g in groups]
    return out


STAMPS = tuple((k, bright, parity, neg) for neg in (False, True) for bright in (True, False) for parity in (0, 1)
               for k in range(16))


def _family_a():
    cases = []
    for inst, size in GEO_A.items():
        # positives and negatives alternate, and the slots are rotated so that the edge slots see both
        order = [s for pair in zip(STAMPS[:64], STAMPS[64:]) for s in pair]
        n = -1
        while order:
            n += 1
            slots = _slots(size, n)
            slots = slots[7 * n % len(slots):] + slots[:7 * n % len(slots)]
            img = _blank(size)
            placed = []
            todo, order = order[:len(slots)], order[len(slots):]
            for (cell, group, y), (k, bright, parity, neg) in zip(slots, todo):
                tx, ty, ww, wh = window(size, cell)
                x = group[parity]
                stamp(img, tx + x, ty + y, k, bright, cut=(0 if k % 2 else 8) if neg else None)
                placed.append(dict(k=k, bright=bright, parity=parity, neg=neg, cell=cell, x=x, y=y, X=tx + x, Y=ty + y,
                                   edge=(x == 0, x == ww - 1, y == 0, y == wh - 1)))
            muts = [("arc", p["k"], p["bright"]) for p in placed if not p["neg"]]
            for th in ((L.INI, L.MIN), (20, 20), (7, 7)):
                cases.append(_case(f"A {inst} image {n} th {th}", "A", size, img.copy(), ("arc",) if th[0] != th[1] else ("arc, one threshold",),
                                   muts if th[0] != th[1] else muts[:1], th=th, stamps=placed))
    return cases


# ---- B. thresholds
def _centre(size, cell, dx=0, dy=0):
    tx, ty, ww, wh = window(size, cell)
    return tx + ww // 2 + dx, ty + wh // 2 + dy


def _dots(size, dots, v=BG):
    """dots: (cell, dx, dy, value) relative to the cell window's centre, value absolute."""
    img = _blank(size, v)
    at = []
    for cell, dx, dy, val in dots:
        x, y = _centre(size, cell, dx, dy)
        img[y, x] = val
        at.append((x, y))
    return img, at


def _rows(at, resp):
    return [(x, y, r) for (x, y), r in zip(at, resp) if r is not None]


def _family_b():
    cases = []
    for inst, size in GEO_22.items():
        img, at = _dots(size, [(c, 0, 0, BG + v) for c, v in enumerate((7, 8, 20, 21))])
        cases.append(_case(f"B {inst} dots +7 +8 +20 +21", "B", size, img, ("threshold sides",), (("th_ge",),),
                           _rows(at, (None, 7, 19, 20))))
        img, at = _dots(size, [(0, -6, 0, BG + 20), (0, 6, 0, BG + 40)])
        cases.append(_case(f"B {inst} +20 beside +40", "B", size, img, ("iniTh side, no fallback",), (("th_ge",),),
                           _rows(at, (None, 39))))
        img, at = _dots(size, [(0, -6, 0, BG + 20), (0, 6, 0, BG + 8)])
        cases.append(_case(f"B {inst} +20 beside +8", "B", size, img, ("iniTh side, fallback",), (("th_ge",),),
                           _rows(at, (19, 7))))
        # the star of the lane cases: an A pair (bound 30) that is no iniTh corner (M = 15)
        img, at = _dots(size, [(0, 6, 0, BG + 8), (0, -6, 0, BG + 30)] +
                        [(0, -6 + a, b, BG + 15) for a in (-2, 2) for b in (-2, 2)])
        cases.append(_case(f"B {inst} star beside +8", "B", size, img, ("A pair without iniTh corner",), (),
                           _rows(at, (7, 14, 14, 14, 14, 14))))
        ends = [(0, 0, 0, 255), (1, 0, 0, 254), (2, 0, 0, 1), (3, 0, 0, 2)]
        for th, resp in (((254, 254), (254, None, None, None)), ((255, 255), (None,) * 4),
                         ((254, 253), (254, 253, None, None)), ((255, 0), (254, 253, None, 1)),
                         ((0, 0), (254, 253, None, 1)), ((20, 0), (254, 253, None, 1)),
                         ((7, 20), (254, 253, None, None))):
            img, at = _dots(size, ends, 0)
            muts = {(254, 254): (("th_ge",),), (255, 255): (("th_ge",),)}.get(th, ())
            if th in ((255, 0), (0, 0), (20, 0)):
                muts = (("nms_ge",),)      # the value-1 pixel: score 0, kept only by a maximum that is not strict
            cases.append(_case(f"B {inst} ends th {th}", "B", size, img, (f"threshold ends {th}",), muts,
                               _rows(at, resp), th=th))
        img, at = _dots(size, [(0, 0, 0, 0)], 255)
        cases.append(_case(f"B {inst} dark 255 th (254, 254)", "B", size, img, ("dark side, M = 255",), (),
                           _rows(at, (254,)), th=(254, 254)))
        cases.append(_case(f"B {inst} dark 255 th (255, 255)", "B", size, img.copy(), ("dark side, threshold 255",),
                           (("th_ge",),), [], th=(255, 255)))
    return cases


# ---- C. NMS
def _family_c():
    cases = []
    for inst, size in GEO_22.items():
        for scen in ("weaker", "tie, fallback", "tie, no fallback"):
            for parity in (0, 1):
                for half in (0, 1):
                    dirs = DIRS[4 * half:4 * half + 4]
                    img, exp = _blank(size), []
                    for cell, (dx, dy) in enumerate(dirs):
                        tx, ty, ww, wh = window(size, cell)
                        x, y = tx + (ww // 2 & ~1) + parity, ty + wh // 2     # the weaker (or first) pixel
                        img[y, x] = BG + (25 if scen == "weaker" else 30)
                        img[y + dy, x + dx] = BG + 30
                        if scen == "weaker":
                            exp.append((x + dx, y + dy, 29))
                        else:
                            v = 10 if scen == "tie, fallback" else 40
                            img[y - 8, x - 8] = BG + v
                            exp.append((x - 8, y - 8, v - 1))
                    muts = {"weaker": [("nms_dir", d) for d in dirs], "tie, fallback": [("nms_ge",), ("fallback_pre",)],
                            "tie, no fallback": [("nms_ge",)]}[scen]
                    cases.append(_case(f"C {inst} {scen}, pixel {parity}, directions {4 * half}-{4 * half + 3}", "C", size,
                                       img, (f"NMS {scen}",), muts, exp, dirs=dirs, parity=parity))
    return cases


# ---- D. windows
def _family_d():
    cases = []
    sizes = list(GEO_22.items()) + [((48, 12), s) for s in GEO_WIDTHS[1:]] + list(GEO_ODD_64.items())
    for inst, size in sizes:
        w, h = size
        t0, t1, t2 = window(size, 0), window(size, 1), window(size, 2)
        bx, by = t0[0] + t0[2] - 1, t0[1] + t0[3] - 1      # the last column / row of cell 0's window
        assert t1[0] == bx + 1 and t2[1] == by + 1, "adjacent windows tile the level"
        tag = f"D {inst} {w}x{h}"
        ymid, xmid = t0[1] + t0[3] // 2, t0[0] + t0[2] // 2
        pairs = {
            "vertical and horizontal boundary": ([((bx, ymid), (bx + 1, ymid)), ((xmid, by), (xmid, by + 1))],
                                                 [("nms_across",), ("window", "r"), ("window", "b")]),
            "corner diagonal": ([((bx, by), (bx + 1, by + 1))], [("nms_across",)]),
            "corner antidiagonal": ([((bx + 1, by), (bx, by + 1))], [("nms_across",)]),
        }
        for name, (pp, muts) in pairs.items():
            img, exp = _blank(size), []
            for (xa, ya), (xb, yb) in pp:
                img[ya, xa], img[yb, xb] = BG + 25, BG + 30
                exp += [(xa, ya, 24), (xb, yb, 29)]
            cases.append(_case(f"{tag} {name}", "D", size, img, ("cell boundary",) + (("cell boundary, odd width",) if t0[2] % 2 else ()),
                               muts, exp, rem=geometry(size)["rem"][0]))
        # the level's outer window edges: the + 30 dots lie in no window
        y3 = window(size, 3)[1] + window(size, 3)[3] // 2
        x3 = window(size, 3)[0] + window(size, 3)[2] // 2
        outer = [((w - 20, y3), (w - 19, y3)), ((x3, h - 20), (x3, h - 19)), ((xmid, 19), (xmid, 18)), ((19, ymid), (18, ymid))]
        img, exp = _blank(size), []
        for (xa, ya), (xb, yb) in outer:
            img[ya, xa], img[yb, xb] = BG + 25, BG + 30
            exp.append((xa, ya, 24))
        last = geometry(size)["ncells"] - 1
        cases.append(_case(f"{tag} outer edges", "D", size, img, ("outer window edge", f"rem {geometry(size)['rem'][last]}"),
                           [("window", s) for s in "rbtl"] + [("nms_across",)], exp, rem=geometry(size)["rem"][last]))
    return cases


# ---- E. one-pass path
def stripes(size):
    w, h = size
    yy, xx = np.mgrid[:h, :w]
    return np.where((xx + yy) % 6 == 0, BG + 28, BG).astype(np.uint8)


def _find_e(size):
    """The first off-stripe pixel near the middle of cell 0's window that, lowered by 10, is the level's only
    candidate, and a second one that, raised by 60, replaces it."""
    tx, ty, ww, wh = window(size, 0)
    base = stripes(size)
    for y in range(ty + wh // 2, ty + wh - 4):
        for x in range(tx + ww // 2, tx + ww - 4):
            if (x + y) % 6 in (0, 3):
                continue
            low = base.copy()
            low[y, x] -= 10
            if restate(low) != [(x - 16, y - 16, 9)]:
                continue
            for y2 in range(ty + 4, ty + wh // 2 - 4):
                for x2 in range(tx + 4, tx + ww // 2 - 4):
                    if (x2 + y2) % 6 in (0, 3):
                        continue
                    both = low.copy()
                    both[y2, x2] += 60
                    got = restate(both)
                    if len(got) == 1 and got[0][:2] == (x2 - 16, y2 - 16):
                        return (x, y), (x2, y2), got[0][2]
    raise AssertionError(f"no one-pass pixels at {size}")


def _family_e():
    cases = []
    for inst, size in GEO_22.items():
        (x, y), (x2, y2), r2 = _find_e(size)
        base = stripes(size)
        cases.append(_case(f"E {inst} stripes", "E", size, base.copy(), ("one-pass, nothing kept",), (), []))
        low = base.copy()
        low[y, x] -= 10
        cases.append(_case(f"E {inst} stripes, one pixel - 10", "E", size, low.copy(), ("one-pass, minTh list copied",),
                           (("onepass_never",),), [(x, y, 9)]))
        low[y2, x2] += 60
        cases.append(_case(f"E {inst} stripes, - 10 and + 60", "E", size, low, ("one-pass, minTh list discarded",),
                           (("onepass_always",),), [(x2, y2, r2)]))
    return cases


CASES = tuple(_family_a() + _family_b() + _family_c() + _family_d() + _family_e())
IDS = [c.name for c in CASES]
# the kernel's classes of NMS neighbour, by the weaker pixel's position in its pair (0 / 1) and the direction
NMS_CLASS = {(p, d): ("inside the pair" if d == ((1, 0), (-1, 0))[p] else
                      "next pair in the row" if d[1] == 0 else "row above or below") for p in (0, 1) for d in DIRS}


def by_name(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def candidates(case: Case) -> np.ndarray:
    return O.level_candidates(O.OracleExtractor(**case.params).p, case.img)


@functools.lru_cache(maxsize=None)
def ref(case: Case) -> tuple:
    """The oracle's keypoints and descriptors of the case's image."""
    return O.OracleExtractor(**case.params).extract(case.img)


@functools.lru_cache(maxsize=None)
def counts(case: Case) -> tuple:
    """lane_counts of every cell (minTh < iniTh only): the path each cell takes."""
    D = model()
    M, bound = D.maps(case.img)
    cs = grid(case.size)
    cap = max(D.pair_cap(c) for c in cs)
    return tuple(D.lane_counts(M, bound, c, cap, *case.th) for c in cs)
