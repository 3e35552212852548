"""Fixtures that put keypoints on k_orb's decision points (tests/test_gpu_orb_edges.py) and their CPU
pre-conditions (tests/test_orb_cases_cpu.py): deterministic builders, pure numpy plus the oracle.

k_orb stages a keypoint's 43 x 48 window by dword loads when 25 <= cx and cx + 22 < Lw and byte by byte with
reflect-101 columns otherwise, reflects rows when cy < 21 or cy + 21 >= Lh, re-aligns a dword-staged row by the
misalignment of its first byte (the level's base included: only level 0 has an unaligned base and a pitch that is
not a multiple of 4), and issues loads that end at the buffer's last dword for keypoints in the bottom-right
corner.  FAST keeps keypoints in 19 <= cx <= Lw - 20, 19 <= cy <= Lh - 20, so the classes are columns 19 .. 24 and
Lw - 22 .. Lw - 20 (bytes), rows 19, 20 and Lh - 21, Lh - 20 (reflected), and everything else.

Neighbouring corners suppress each other and the octree may drop one of two keypoints alone in a node, so every
fixture is BUILT AND THEN CHECKED: a builder adds a dot to an image only if the oracle still keeps every keypoint
the image promises, and test_orb_cases_cpu.py asserts the promises again on the finished set.

  * placement set: single 255 pixels (level 0) and 2 x 2 blocks of 255 (level 1, found by a +-2 px search around
    1.2 x the target) on a 100 + U{-3..3} background, whose contrast stays below minThFAST = 7, each with a
    satellite on a diagonal (the angle then steers samples to all four sides) and a 4 px frame of full-range noise
    where only the blur looks; plus four searched cases whose descriptors provably depend on the reflected pixels;
  * orientation set: a 255 centre pixel plus satellites on a flat 100 background, one level: the centre's
    moments are (sum dy (I - 100), sum dx (I - 100)) over its satellites.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import orb_definition as D
from oracle.oracle import OracleExtractor, lib

H, W = 97, 131                      # W * H = 3 mod 4: image slot i of a batch starts at byte offset 3 i mod 4
PLACEMENT_LEVELS = 3
BASE = dict(nfeatures=1000, scaleFactor=1.2, iniThFAST=20, minThFAST=7)
BF, FX = 40.0, 100.0
EDGE = 19                           # no keypoint lies closer to a level's border
NOISE_SEED = 842                    # searched for: see noise_case


def params(nlevels: int) -> dict:
    return dict(BASE, nlevels=int(nlevels))


def level_sizes(nlevels: int) -> list:
    return OracleExtractor(**params(nlevels)).level_sizes(W, H)


class Promise(NamedTuple):
    label: str      # the class this keypoint stands for
    level: int
    cx: int
    cy: int


class Case(NamedTuple):
    name: str
    image: np.ndarray
    nlevels: int
    promises: tuple


class Ref:
    """The oracle's view of one image at this module's parameters."""

    def __init__(self, img: np.ndarray, nlevels: int, prm: dict | None = None):
        ox = OracleExtractor(**(prm or params(nlevels)))
        self.kps, self.desc = ox.extract(img)
        self.pyramid = ox.pyramid()
        self.tables = ox.tables()
        self.nlevels = nlevels
        sc = self.tables["scale"][self.kps["octave"]]
        self.level = self.kps["octave"].astype(int)
        self.cx = np.rint(self.kps["x"] / sc).astype(int)
        self.cy = np.rint(self.kps["y"] / sc).astype(int)
        # position inside the level's run of the level-major output: even = A, odd = B of a wave's pair
        self.pos = np.zeros(len(self.kps), int)
        for l in range(nlevels):
            m = self.level == l
            self.pos[m] = np.arange(int(m.sum()))

    def index(self) -> dict:
        return {(int(l), int(x), int(y)): i for i, (l, x, y) in enumerate(zip(self.level, self.cx, self.cy))}


def staging_class(lw: int, lh: int, cx: int, cy: int) -> str:
    """k_orb's staging path of a keypoint at level pixel (cx, cy) of an lw x lh level."""
    cols = "dword columns" if 25 <= cx and cx + 22 < lw else "byte columns"
    rows = "rows inside" if 21 <= cy and cy + 21 < lh else "reflected rows"
    return f"{cols}, {rows}"


def describe_keypoint(case: Case, ref: Ref, i: int) -> str:
    """Image, level coordinates and class of keypoint i, for a failure message."""
    l, cx, cy = int(ref.level[i]), int(ref.cx[i]), int(ref.cy[i])
    lh, lw = ref.pyramid[l].shape
    labels = [p.label for p in case.promises if (p.level, p.cx, p.cy) == (l, cx, cy)]
    return (f"image {case.name!r}, level {l} ({lw} x {lh}), keypoint {i} at ({cx}, {cy}), position {int(ref.pos[i])} "
            f"of its level: {staging_class(lw, lh, cx, cy)}; {', '.join(labels) if labels else 'not a promised one'}")


# ---- the placement set ------------------------------------------------------------------------------------------
FRAME = 4  # px of full-range noise along the image's border


def background(seed: int) -> np.ndarray:
    """100 + U{-3..3} inside (below minThFAST = 7: no corner of its own), and a frame of FRAME px of uniform 0 .. 255
    noise.  FAST never looks at the outer 16 px of a level and the centroid disc of a keypoint (>= 19 px from the
    border, radius 15) never reaches the frame, so the frame changes neither the keypoints nor their angles; but
    a 7 x 7 blur within 6 px of the border does, and so do the pixels reflected across it."""
    rng = np.random.default_rng(seed)
    img = (100 + rng.integers(-3, 4, (H, W))).astype(np.uint8)
    noise = rng.integers(0, 256, (H, W)).astype(np.uint8)
    inner = np.zeros((H, W), bool)
    inner[FRAME:H - FRAME, FRAME:W - FRAME] = True
    return np.where(inner, img, noise)


def level0_targets() -> list:
    """(label, cx, cy) on level 0: the full product of the column and row classes' edges, then the alignment runs
    (four consecutive columns at both ends of the dword range: every misalignment, with and without reflected
    rows; the right-hand run at row Lh - 22 issues the loads that end at the buffer's bound)."""
    cols = [19, 24, 25, W - 23, W - 22, W - 20]
    rows = [19, 20, 21, H - 22, H - 21, H - 20]
    out = {}
    for cy in rows:
        for cx in cols:
            out[(cx, cy)] = "product"
    for cy in (20, 21, H - 22, H - 21):
        for cx in list(range(25, 29)) + list(range(W - 26, W - 22)):
            out[(cx, cy)] = out.get((cx, cy), "") + ("+run" if (cx, cy) in out else "run")
    return [(lab, cx, cy) for (cx, cy), lab in out.items()]


EXTREME_DWORD = [(cx, cy) for cx in (25, W - 23) for cy in (21, H - 22)]  # the four extreme dword placements


def level1_targets() -> list:
    lw, lh = level_sizes(PLACEMENT_LEVELS)[1]
    return [(19, 19), (24, 20), (25, 21), (lw - 23, lh - 22), (lw - 22, lh - 21), (lw - 20, lh - 20),
            (lw - 26, lh - 22), (lw - 25, lh - 22), (lw - 24, lh - 22)]


def reflected_axes(lw: int, lh: int, cx: int, cy: int) -> tuple:
    """The axes along which a descriptor sample of a keypoint at (cx, cy) can need a pixel from beyond the level:
    samples reach +-18 and the blur 3 more."""
    return tuple(ax for ax, lo, n in (("columns", cx, lw), ("rows", cy, lh)) if lo - 21 < 0 or lo + 21 >= n)


def border_dependence(ref: "Ref", i: int) -> dict:
    """Per axis of reflected_axes(): does keypoint i's descriptor change when the level is extended along that
    axis by replicating the edge pixel AND when it is extended by zeros, instead of reflect-101?  True means a
    kernel that reflects wrongly along that axis cannot give this keypoint's descriptor.  (The descriptor is
    orb_definition's, with the oracle's cos / sin so that the fixtures do not depend on the host's libm.)"""
    l, cx, cy = int(ref.level[i]), int(ref.cx[i]), int(ref.cy[i])
    lvl = ref.pyramid[l]
    rad = np.float32(ref.kps["angle"][i]) * np.float32(math.pi / 180.0)
    ab = (np.float32(lib().oracle_cosf(float(rad))), np.float32(lib().oracle_sinf(float(rad))))
    out = {}
    for axis in reflected_axes(lvl.shape[1], lvl.shape[0], cx, cy):
        out[axis] = all(
            D.descriptor(D.blur7(lvl, **{("col_mode" if axis == "columns" else "row_mode"): mode}), cx, cy,
                         ref.kps["angle"][i], ab=ab) != ref.desc[i].tobytes() for mode in ("edge", "constant"))
    return out


def _kept(img: np.ndarray, nlevels: int) -> dict:
    return Ref(img, nlevels).index()


class _Builder:
    """One image under construction: its marks (level-0 pixels set to 255, those of different placements at least
    8 px apart) and promises."""

    def __init__(self, name: str, seed: int):
        self.name, self.img, self.marks, self.promises = name, background(seed), [], []

    def far_enough(self, x: int, y: int, gap: int = 8) -> bool:
        return all(max(abs(x - mx), abs(y - my)) >= gap for mx, my in self.marks)

    def try_add(self, pixels, promise: Promise) -> bool:
        """Sets `pixels` to 255 if the oracle then keeps the new promise and every earlier one."""
        trial = self.img.copy()
        for x, y in pixels:
            trial[y, x] = 255
        kept = _kept(trial, PLACEMENT_LEVELS)
        if not all((p.level, p.cx, p.cy) in kept for p in self.promises + [promise]):
            return False
        self.img = trial
        self.marks += list(pixels)
        self.promises.append(promise)
        return True

    def case(self) -> Case:
        return Case(self.name, self.img, PLACEMENT_LEVELS, tuple(self.promises))


# Few samples reach the pixels reflected across a level's border, through one or two of the blur's outer taps, so
# for most border keypoints a wrong reflection changes no descriptor bit (test_orb_cases_cpu.py counts them).  These
# four (background seed, satellite diagonal) were searched for, one per side: the keypoint's descriptor changes when
# the level is extended by the edge pixel and when it is extended by zeros (border_dependence).
REFLECTION = (("left", 19, 48, 1014, (-1, -1)), ("right", W - 20, 48, 1006, (-1, 1)),
              ("top", 65, 19, 1003, (1, 1)), ("bottom", 65, H - 20, 1010, (-1, 1)))


def _reflection_cases():
    for side, cx, cy, seed, (sx, sy) in REFLECTION:
        img = background(seed)
        img[cy, cx] = img[cy + 8 * sy, cx + 8 * sx] = 255
        yield Case(f"reflection {side}", img, PLACEMENT_LEVELS, (Promise(f"depends on the {side} reflection", 0, cx, cy),))


DIAGONALS = ((1, 1), (-1, 1), (1, -1), (-1, -1))


@functools.lru_cache(maxsize=None)
def placement_set() -> tuple:
    """Cases covering level0_targets(), level1_targets() and both wave-pair halves of EXTREME_DWORD.  Every
    target comes with a satellite on a diagonal (8 px away on level 0, a 2 x 2 block 10 px away for level 1): an
    angle near an odd multiple of 45 degrees turns the pattern's corner points (+-13, +-13) onto the axes, so
    that samples reach 18 px up, down, left and right, which is where the reflected pixels and the last staged
    row and column are.  Shared among the tests of a run; read-only."""
    builders: list[_Builder] = []

    def inside(pixels):
        return all(FRAME <= x < W - FRAME and FRAME <= y < H - FRAME for x, y in pixels)

    def place(make_pixels, promise, gap):
        fresh = _Builder(f"placement {len(builders)}", 100 + len(builders))
        for b in builders + [fresh]:
            for pixels in make_pixels():
                if inside(pixels) and all(b.far_enough(x, y, gap) for x, y in pixels) and b.try_add(pixels, promise):
                    if b is fresh:
                        builders.append(b)
                    return
        raise AssertionError(f"cannot place {promise}")

    for lab, cx, cy in level0_targets():
        place(lambda: ([(cx, cy), (cx + 8 * sx, cy + 8 * sy)] for sx, sy in DIAGONALS),
              Promise(f"level 0 {lab}", 0, cx, cy), 8)
    for tx, ty in level1_targets():
        bx, by = round(1.2 * tx), round(1.2 * ty)

        def blocks():
            for sx, sy in DIAGONALS:
                for dy in (0, -1, 1, -2, 2):
                    for dx in (0, -1, 1, -2, 2):
                        yield [(x + i, y + j) for x, y in ((bx + dx, by + dy), (bx + dx + 10 * sx, by + dy + 10 * sy))
                               for j in (0, 1) for i in (0, 1)]
        place(blocks, Promise("level 1", 1, tx, ty), 12)
    cases = [b.case() for b in builders] + list(_reflection_cases())

    # both halves of a wave's pair for the four extreme dword placements: where one parity is missing, a copy of
    # an image that holds the placement with one more dot far away from every other, kept if the oracle shows the
    # position's parity flipped and every promise still held
    for cx, cy in EXTREME_DWORD:
        have, holders = set(), []
        for c in cases:
            r = Ref(c.image, c.nlevels)
            i = r.index().get((0, cx, cy))
            if i is not None and any((p.level, p.cx, p.cy) == (0, cx, cy) for p in c.promises):
                have.add(int(r.pos[i]) % 2)
                holders.append(c)
        for parity in {0, 1} - have:
            cases.append(_parity_variant(holders, cx, cy, parity, len(cases)))
    return tuple(cases)


def _parity_variant(holders, cx: int, cy: int, parity: int, n: int) -> Case:
    for holder in holders:
        marks = [(x, y) for y, x in zip(*np.nonzero(holder.image == 255))]
        for y in range(EDGE, H - EDGE, 3):
            for x in range(EDGE, W - EDGE, 3):
                if any(max(abs(x - mx), abs(y - my)) < 10 for mx, my in marks):
                    continue
                trial = holder.image.copy()
                trial[y, x] = 255
                ref = Ref(trial, holder.nlevels)
                kept = ref.index()
                if (all((p.level, p.cx, p.cy) in kept for p in holder.promises)
                        and ref.pos[kept[(0, cx, cy)]] % 2 == parity):
                    promises = tuple(p._replace(label=p.label + f", pair half {'AB'[parity]}")
                                     if (p.level, p.cx, p.cy) == (0, cx, cy) else p for p in holder.promises)
                    return Case(f"placement {n} (parity of ({cx}, {cy}))", trial, holder.nlevels, promises)
    raise AssertionError(f"no far-away dot flips the parity of ({cx}, {cy})")


# ---- the orientation set ----------------------------------------------------------------------------------------
CENTRES = [(x, y) for y in (28, 68) for x in (25, 65, 105)]  # 40 px apart: a group's satellites (<= 12 px) stay
                                                             # outside every other centre's 15 px disc
SAT = 240   # the satellites are dimmer than the centre: its FAST score wins where the octree keeps one of a node
RING = [(dx, dy) for dy in range(-12, 13) for dx in range(-12, 13) if 64 <= dx * dx + dy * dy <= 144]


def group_moments(sats) -> tuple[int, int]:
    """(m01, m10) of a centre whose satellites are (dx, dy, value) on the flat 100 background."""
    return sum(dy * (v - 100) for _, dy, v in sats), sum(dx * (v - 100) for dx, _, v in sats)


def _octant_groups() -> list:
    """Per multiple of 45 degrees two groups, one within 2 degrees on each side of it: a satellite on the axis
    or diagonal and a second, dimmer one found by search over the four axis offsets and brightness 101 .. 110."""
    main = [(10, 0), (8, 8), (0, 10), (-8, 8), (-10, 0), (-8, -8), (0, -10), (8, -8)]
    out = []
    for k, (mx, my) in enumerate(main):
        for side in (-1, 1):
            found = None
            for v in range(101, 111):
                for dx, dy in ((8, 0), (0, 8), (-8, 0), (0, -8)):
                    sats = ((mx, my, SAT), (dx, dy, v))
                    m01, m10 = group_moments(sats)
                    off = (float(D.fast_atan2(m01, m10)) - 45.0 * k + 180.0) % 360.0 - 180.0
                    if found is None and 0.0 < side * off < 2.0:
                        found = (f"octant boundary {45 * k} {'below' if side < 0 else 'above'}", sats)
            assert found, (k, side)
            out.append(found)
    return out


def _fixed_groups() -> list:
    g = [("zero moment", ())]
    g += [(f"axis {name}", ((dx, dy, SAT),)) for name, dx, dy in (("+x", 8, 0), ("+y", 0, 8), ("-x", -8, 0),
                                                                   ("-y", 0, -8))]
    g += [(f"diagonal ({dx}, {dy})", ((dx, dy, SAT),)) for dx, dy in ((8, 8), (-8, 8), (-8, -8), (8, -8))]
    return g + _octant_groups()


RING_GROUPS = 150


def _ring_groups() -> list:
    """Satellite offsets of radius 8 .. 12 and brightness 101 .. 255, one or two per centre."""
    rng = np.random.default_rng(2024)
    out = []
    while len(out) < RING_GROUPS:
        sats = []
        for _ in range(1 + len(out) % 2):
            dx, dy = RING[int(rng.integers(len(RING)))]
            if all(max(abs(dx - sx), abs(dy - sy)) >= 8 for sx, sy, _ in sats):
                sats.append((dx, dy, int(rng.integers(101, 256))))
        if group_moments(sats) != (0, 0):
            out.append(("ring", tuple(sats)))
    return out


def _draw(groups) -> np.ndarray:
    img = np.full((H, W), 100, np.uint8)
    for (cx, cy), (_, sats) in zip(CENTRES, groups):
        img[cy, cx] = 255
        for dx, dy, v in sats:
            img[cy + dy, cx + dx] = v
    return img


@functools.lru_cache(maxsize=None)
def _orientation() -> tuple:
    pending = _fixed_groups() + _ring_groups()
    cases, sats_of = [], {}
    while pending:
        chosen, rest = [], []
        for g in pending:
            if len(chosen) < len(CENTRES):
                kept = _kept(_draw(chosen + [g]), 1)
                if all((0, cx, cy) in kept for (cx, cy), _ in zip(CENTRES, chosen + [g])):
                    chosen.append(g)
                    continue
            rest.append(g)
        assert chosen, "no group of the remaining ones keeps its centre alone"
        name = f"orientation {len(cases)}"
        promises = tuple(Promise(lab, 0, cx, cy) for (cx, cy), (lab, _) in zip(CENTRES, chosen))
        for (cx, cy), (_, sats) in zip(CENTRES, chosen):
            sats_of[(name, cx, cy)] = sats
        cases.append(Case(name, _draw(chosen), 1, promises))
        pending = rest
    return tuple(cases), sats_of


def orientation_set() -> tuple:
    """One-level cases of up to six centre-plus-satellite groups; every promise is a group's centre, labelled
    with its class.  A group whose centre the oracle would not keep next to the image's earlier groups goes to a
    later image.  Shared among the tests of a run; read-only."""
    return _orientation()[0]


def orientation_groups() -> dict:
    """(case name, cx, cy) of every promised centre -> its satellites (dx, dy, value)."""
    return _orientation()[1]


# ---- the noise image ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise_case() -> Case:
    """131 x 96 uniform noise, 3 levels, about 300 keypoints all over the levels.  The seed is the first of
    0 .. 4000 at which rounding the product px * b before the sum (orb_definition's fused=False) moves a sample
    across a pixel boundary AND changes a descriptor bit: a coordinate must lie within about an ulp of a
    half-integer for that, which about one seed in 130 has, and one in 350 with a changed bit."""
    img = np.random.default_rng(NOISE_SEED).integers(0, 256, (96, 131)).astype(np.uint8)
    return Case("noise", img, 3, ())


NOISE_PARAMS = dict(nfeatures=300, scaleFactor=1.2, iniThFAST=20, minThFAST=7, nlevels=3)


@functools.lru_cache(maxsize=None)
def ref(case_name: str) -> Ref:
    """The oracle's reference of a case of either set or of the noise image, computed once."""
    if case_name == "noise":
        return Ref(noise_case().image, 3, NOISE_PARAMS)
    for c in placement_set() + orientation_set():
        if c.name == case_name:
            return Ref(c.image, c.nlevels)
    raise KeyError(case_name)
