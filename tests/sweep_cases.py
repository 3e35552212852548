"""Inputs of the small-geometry sweep (tests/test_gpu_sweep.py) and of its CPU pre-conditions
(tests/test_sweep_cases_cpu.py): image contents, geometry lists and the mixed batch, pure numpy and
deterministic by seed, plus the oracle / restatement reference of an image pair, computed once per input.

The geometries are tiny on purpose (an image of about 100 x 65 costs the oracle 2-3 ms), so that every image
and every pair of every case is compared, never a sample."""
from __future__ import annotations

import functools

import numpy as np

from oracle import stereo_oracle
from oracle.oracle import OracleExtractor
from pyorbslam_amd import synth

# extractor parameters of every case (nlevels comes with the geometry) and the stereo constants
BASE = dict(nfeatures=300, scaleFactor=1.2, iniThFAST=20, minThFAST=7)
BF, FX = 40.0, 100.0


def params(nlevels: int) -> dict:
    return dict(BASE, nlevels=int(nlevels))


# ---- contents: (h, w) uint8, C-contiguous -------------------------------------------------------------------
def natural_pair(seed: int, h: int, w: int) -> tuple[np.ndarray, np.ndarray]:
    return synth.make_pair(seed, w, h, dmax=8, block=8)


def natural(seed: int, h: int, w: int) -> np.ndarray:
    return natural_pair(seed, h, w)[0]


def noise(seed: int, h: int, w: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def coarse(seed: int, h: int, w: int) -> np.ndarray:
    """Four grey levels 60 apart: many equal FAST scores, and pixel differences that are exact multiples of
    iniTh = 20 (the `v +- th` comparisons at equality)."""
    return np.array([20, 80, 140, 200], np.uint8)[np.random.default_rng(seed).integers(0, 4, (h, w))]


def binary(seed: int, h: int, w: int) -> np.ndarray:
    """0 / 255 at p = 0.5: v + th and v - th saturate."""
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def lattice(h: int, w: int) -> np.ndarray:
    """A bright dot every 4th pixel of every 4th row on black: isolated corners, all with one score."""
    img = np.zeros((h, w), np.uint8)
    img[::4, ::4] = 255
    return img


def flat(h: int, w: int, value: int = 100) -> np.ndarray:
    return np.full((h, w), value, np.uint8)


def shifted(img: np.ndarray, k: int) -> np.ndarray:
    """The right view of `img` at disparity k: what the left shows at column x stands at column x - k (the k
    columns that leave on the left come back on the right)."""
    return np.ascontiguousarray(np.roll(img, -int(k), axis=1))


CONTENT_ORDER = ("noise", "flat", "natural", "coarse")  # the order on one handle: dense -> nothing -> dense


def content(name: str, seed: int, h: int, w: int) -> np.ndarray:
    if name == "flat":
        return flat(h, w)
    if name == "lattice":
        return lattice(h, w)
    return {"noise": noise, "natural": natural, "coarse": coarse, "binary": binary}[name](seed, h, w)


# ---- geometry lists: (h, w, nlevels) ------------------------------------------------------------------------
# 36 consecutive widths: every w mod 30 (the last FAST cell column), w mod 4 (dword tails), and with the two
# heights every W*H mod 4
WIDTHS = [(h, w, 3) for h in (96, 97) for w in range(96, 132)]
# 36 consecutive heights from the lowest that yields a keypoint: at the low end only level 0 has FAST cells,
# the other levels are still resized and sheared
HEIGHTS = [(h, w, 4) for w in (130, 131) for h in range(62, 98)]
# level-1 widths 253, 257, 409, 413, 505: ceil(w / 4) mod 64 = 0, 1, 39, 40, 63, around the resize launcher's
# remainder-wave rule (taken for 1 .. 39)
RESIZE_TAILS = [(76, w, 3) for w in (304, 308, 491, 496, 606)]
RESIZE_TAIL_RESIDUES = (0, 1, 39, 40, 63)
LISTS = {"widths": WIDTHS, "heights": HEIGHTS, "resize_tails": RESIZE_TAILS}


# ---- references ---------------------------------------------------------------------------------------------
class ImageRef:
    """The oracle's view of one image: keypoints, descriptors, pyramids and the level tables."""

    def __init__(self, img: np.ndarray, nlevels: int):
        ox = OracleExtractor(**params(nlevels))
        self.kps, self.desc = ox.extract(img)
        self.pyramid = ox.pyramid()
        self.sheared = ox.sheared_pyramid()
        self.tables = ox.tables()

    def levels_with_keypoints(self) -> set:
        return set(int(o) for o in np.unique(self.kps["octave"]))


class PairRef:
    """The restatement's stereo result of a pair: (status, value) encodings of mvuRight and mvDepth, and the
    chosen right index per left keypoint."""

    def __init__(self, left: ImageRef, right: ImageRef):
        t = left.tables
        u, d, m = stereo_oracle.compute_stereo_matches(left.kps, right.kps, left.desc, right.desc, left.sheared,
                                                       right.sheared, t["scale"], t["inv_scale"], BF, np.float32(FX))
        self.status, self.u_right = stereo_oracle.encode(u)
        self.status_d, self.depth = stereo_oracle.encode(d)
        self.match_r = m


def encode_gpu(res: dict, kps_left: np.ndarray):
    """A GPU stereo result (status / u_right / depth arrays) in PairRef's encoding, through the host code that
    builds the reference's lists."""
    from pyorbslam_amd.frame import to_reference_lists
    u, d = to_reference_lists(res, kps_left, BF)
    return stereo_oracle.encode(u) + stereo_oracle.encode(d)


def assert_image(kps, desc, ref: ImageRef, what) -> None:
    assert len(kps) == len(ref.kps), (what, len(kps), len(ref.kps))
    assert kps.tobytes() == ref.kps.tobytes(), what
    assert np.array_equal(np.asarray(desc).reshape(-1, 32), ref.desc), what


def assert_stereo(res: dict, kps_left, ref: PairRef, what) -> None:
    su, vu, sd, vd = encode_gpu(res, kps_left)
    assert np.array_equal(su, ref.status) and np.array_equal(sd, ref.status_d), what
    assert np.array_equal(vu, ref.u_right) and np.array_equal(vd, ref.depth), what
    assert np.array_equal(res["match_r"], ref.match_r), what


# ---- the mixed batch ----------------------------------------------------------------------------------------
MIXED_GEOMETRIES = [(96, 131), (97, 130), (97, 129)]  # W*H = 0, 2 and 1 mod 4
MIXED_NLEVELS = 3
PAIR_KINDS = ("natural", "noise", "lattice", "binary", "coarse", "flat_noise", "noise_flat", "flat_flat")
BOTH_SIDES = ("natural", "noise", "lattice", "binary", "coarse")  # the kinds with keypoints left and right


SEED_PERIOD = len(PAIR_KINDS) ** 2


def pair_kind(p: int) -> str:
    """Every run of 8 pairs holds the 8 kinds; each run starts one kind later, so that over a long batch every
    kind meets every residue of the image's byte offset (2 p W H) mod 4."""
    return PAIR_KINDS[(p + p // len(PAIR_KINDS)) % len(PAIR_KINDS)]


def make_pair_of_kind(kind: str, seed: int, h: int, w: int) -> tuple[np.ndarray, np.ndarray]:
    if kind == "natural":
        return natural_pair(seed, h, w)
    if kind == "noise":
        n = noise(seed, h, w)
        return n, shifted(n, 3)
    if kind == "lattice":
        return lattice(h, w), lattice(h, w)
    if kind == "binary":
        b = binary(seed, h, w)
        return b, b.copy()
    if kind == "coarse":
        c = coarse(seed, h, w)
        return c, shifted(c, 3)
    if kind == "flat_noise":
        return flat(h, w), noise(seed, h, w)
    if kind == "noise_flat":
        return noise(seed, h, w), flat(h, w)
    assert kind == "flat_flat", kind
    return flat(h, w, 100 + seed % 50), flat(h, w, 60)


class MixedBatch:
    """n_pairs pairs of the mixed kinds at one geometry: images (2P, h, w), and per image / pair the oracle's
    and the restatement's results (images and pairs with equal pixels share one reference object)."""

    def __init__(self, h: int, w: int, n_pairs: int, seed0: int, first: int = 0):
        self.h, self.w, self.n_pairs = h, w, n_pairs
        self.kinds = [pair_kind(first + p) for p in range(n_pairs)]
        self.images = np.empty((2 * n_pairs, h, w), np.uint8)
        for p, kind in enumerate(self.kinds):
            # the seeds repeat with the kinds' rotation (64 pairs), which bounds the reference's cost for a long
            # batch; the device still computes, and the tests still compare, every image and pair
            self.images[2 * p], self.images[2 * p + 1] = make_pair_of_kind(kind, seed0 + p % SEED_PERIOD, h, w)
        cache = {}
        self.image_refs = []
        for img in self.images:
            key = img.tobytes()
            if key not in cache:
                cache[key] = ImageRef(img, MIXED_NLEVELS)
            self.image_refs.append(cache[key])
        pcache = {}
        self.pair_refs = []
        for p in range(n_pairs):
            key = (id(self.image_refs[2 * p]), id(self.image_refs[2 * p + 1]))
            if key not in pcache:
                pcache[key] = PairRef(self.image_refs[2 * p], self.image_refs[2 * p + 1])
            self.pair_refs.append(pcache[key])


@functools.lru_cache(maxsize=None)
def mixed_batch(h: int, w: int, n_pairs: int, seed0: int = 1000, first: int = 0) -> MixedBatch:
    """Pair p is of kind pair_kind(first + p), from seed seed0 + p.  Shared among the tests of one run; treat as
    read-only."""
    return MixedBatch(h, w, n_pairs, seed0, first)
