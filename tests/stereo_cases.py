"""Inputs of the stereo matcher's boundary tests (tests/test_gpu_stereo_edges.py) and of their CPU pre-conditions
(tests/test_stereo_cases_cpu.py): tiny image pairs, pure numpy and deterministic by seed, at which the gates of
Frame.compute_stereo_matches sit next to a result, the list of (pair, extractor parameters, bf, fx) cases with
the names of their goldens (tests/golden/stereo_edges_*.npz, the reference's own outputs), and census(), a
plain walk over a case's inputs that counts how often each gate decides and labels every left keypoint.

With bf = 40 the maximum disparity maxD = bf / (bf / fx) is fx itself, so an integer fx equal to the shift puts
keypoints exactly on `minU <= uR` and on `disparity < maxD`; fx = 100 leaves both gates open and lets the
descriptor threshold, the SAD scan and the sign of the disparity decide."""
from __future__ import annotations

import functools
import json
import math

import numpy as np

import sweep_cases as S
from oracle import stereo_oracle
from oracle.oracle import EDGE, OracleExtractor

H, W, NLEVELS = 97, 131, 3
BF = 40.0
FXS = (2.5, 3.0, 3.5, 4.0, 100.0)
SHIFT = 3
SEED = 1
PARAMS = S.params(NLEVELS)                      # nfeatures = 300: row buckets of at most 64 entries
PARAMS_LONG = dict(PARAMS, nfeatures=1000)      # row buckets of 65 and more: the search's third and later steps

# the unfused row-bucket kernels' geometry: two distinct noise pairs per height
TALL_W, TALL_HEIGHTS, TALL_NLEVELS = 480, (879, 880), 3
TALL_PARAMS = dict(S.BASE, nfeatures=600, nlevels=TALL_NLEVELS)
TALL_SEEDS = (11, 12)


# ---- contents ------------------------------------------------------------------------------------------------
def noisy_shift(img: np.ndarray, k: int, amp: int, seed: int) -> np.ndarray:
    """shifted(img, k) plus uniform pixel noise in [-amp, amp], clipped: descriptors drift towards the 74 / 75
    threshold and the SAD minimum towards the ends of its scan."""
    n = np.random.default_rng(seed).integers(-amp, amp + 1, img.shape)
    return np.clip(S.shifted(img, k).astype(np.int64) + n, 0, 255).astype(np.uint8)


def sparse_right(img: np.ndarray, k: int, first_flat_row: int = 50) -> np.ndarray:
    """shifted(img, k) with the rows from first_flat_row on set to 100: the left keypoints down there meet an
    empty row bucket, those above still match."""
    r = S.shifted(img, k).copy()
    r[first_flat_row:] = 100
    return r


def make_pair(name: str, seed: int = SEED, h: int = H, w: int = W) -> tuple[np.ndarray, np.ndarray]:
    n = S.noise(seed, h, w)
    if name == "noise3":
        return n, S.shifted(n, SHIFT)
    if name == "coarse3":
        c = S.coarse(seed, h, w)
        return c, S.shifted(c, SHIFT)
    if name == "natural":
        return S.natural_pair(seed, h, w)
    if name == "binary_same":
        b = S.binary(seed, h, w)
        return b, b.copy()
    if name == "lattice_same":
        return S.lattice(h, w), S.lattice(h, w)
    if name == "noisy40":
        return n, noisy_shift(n, SHIFT, 40, seed + 100)
    if name == "noisy70":
        return n, noisy_shift(n, SHIFT, 70, seed + 200)
    if name == "noise_same":
        return n, n.copy()
    if name == "noise_m2":
        return n, S.shifted(n, -2)
    assert name == "sparse_right", name
    return n, sparse_right(n, SHIFT)


PAIRS = ("noise3", "coarse3", "natural", "binary_same", "lattice_same", "noisy40", "noisy70", "noise_same",
         "noise_m2", "sparse_right")


# ---- the cases -----------------------------------------------------------------------------------------------
class Case:
    """One (pair, extractor parameters, bf, fx); `golden` names its file, `key` its arrays inside."""

    def __init__(self, pair: str, fx: float, long: bool = False):
        self.pair, self.fx, self.bf, self.long = pair, float(fx), BF, long
        self.params = PARAMS_LONG if long else PARAMS
        self.group = pair + ("_n1000" if long else "")
        self.golden = f"stereo_edges_{self.group}"
        self.key = f"fx{self.fx:g}"
        self.id = f"{self.group}-{self.key}"


# every pair at every fx on the nfeatures = 300 handle; the long-bucket cases need a handle of their own
CASES = [Case(p, fx) for p in PAIRS for fx in FXS]
LONG_CASES = [Case("noise3", fx, long=True) for fx in (3.0, 100.0)]
ALL_CASES = CASES + LONG_CASES
GROUPS = sorted({c.group for c in ALL_CASES})


def cases_of(group: str) -> list:
    return [c for c in ALL_CASES if c.group == group]


@functools.lru_cache(maxsize=None)
def image_ref(group: str, side: int):
    """The oracle's view (S.ImageRef fields) of one side of a group's pair; shared, treat as read-only."""
    c = cases_of(group)[0]
    img = make_pair(c.pair)[side]
    return _ref_of(img, tuple(sorted(c.params.items())))


class _Ref:
    def __init__(self, img: np.ndarray, params: dict):
        ox = OracleExtractor(**params)
        self.image = img
        self.kps, self.desc = ox.extract(img)
        self.sheared = ox.sheared_pyramid()
        self.tables = ox.tables()


@functools.lru_cache(maxsize=None)
def _ref_of_bytes(raw: bytes, shape: tuple, params: tuple) -> _Ref:
    return _Ref(np.frombuffer(raw, np.uint8).reshape(shape).copy(), dict(params))


def _ref_of(img: np.ndarray, params: tuple) -> _Ref:
    return _ref_of_bytes(img.tobytes(), img.shape, params)


def restate(left: _Ref, right: _Ref, bf: float, fx: float):
    """The restatement's result in the goldens' encoding: status, u_right, depth (f64) and match_r."""
    t = left.tables
    u, d, m = stereo_oracle.compute_stereo_matches(left.kps, right.kps, left.desc, right.desc, left.sheared,
                                                   right.sheared, t["scale"], t["inv_scale"], bf, np.float32(fx))
    su, vu = stereo_oracle.encode(u)
    sd, vd = stereo_oracle.encode(d)
    assert np.array_equal(su, sd)
    return su, vu, vd, m


@functools.lru_cache(maxsize=None)
def restated(case_id: str):
    c = next(c for c in ALL_CASES if c.id == case_id)
    return restate(image_ref(c.group, 0), image_ref(c.group, 1), c.bf, c.fx)


@functools.lru_cache(maxsize=None)
def load_golden(group: str) -> dict:
    from conftest import GOLDEN
    z = np.load(GOLDEN / f"stereo_edges_{group}.npz", allow_pickle=False)
    return {k: z[k] for k in z.files}


def golden_of(case: Case) -> dict:
    """status, u_right, depth and the stored census of one case, plus its group's input digests."""
    g = load_golden(case.group)
    out = {k: g[f"{case.key}_{k}"] for k in ("status", "u_right", "depth")}
    out["census"] = json.loads(str(g["meta"]))["census"][case.key]
    for k in ("kps_left_sha", "desc_left_sha", "kps_right_sha", "desc_right_sha"):
        out[k] = str(g[k])
    return out


@functools.lru_cache(maxsize=None)
def tall_pair(h: int, k: int):
    """Pair k of the tall geometry: noise at disparity 3; (left ref, right ref, restated result at fx = 100)."""
    n = S.noise(TALL_SEEDS[k], h, TALL_W)
    prm = tuple(sorted(TALL_PARAMS.items()))
    left, right = _ref_of(n, prm), _ref_of(S.shifted(n, SHIFT), prm)
    return left, right, restate(left, right, BF, 100.0)


# ---- the census ----------------------------------------------------------------------------------------------
# labels of a left keypoint, in the order the method decides; MATCH and ZERO are the golden's statuses 1 and 2,
# every other label is status 0
EMPTY_BUCKET, NO_CANDIDATE, FAR_DESCRIPTOR, STRIP_LEAVES, MIN_AT_END, STEEP_PARABOLA, DISPARITY_OUT, ZERO, MATCH = (
    "empty_bucket", "no_candidate", "far_descriptor", "strip_leaves", "min_at_end", "steep_parabola",
    "disparity_out", "zero", "match")
STATUS_OF_LABEL = {MATCH: 1, ZERO: 2}

COUNTS = ("ur_eq_minu", "disparity_ge_maxd", "accepted_within_1px_of_maxd", "best_74", "best_75",
          "distance_ties_below_75", "sad_min_ties", "bestinc_minus_l", "bestinc_plus_l", "disparity_negative",
          "disparity_zero", "disparity_zero_octave0", "refined_octave0", "refined_octave1", "refined_octave2",
          "left_rows", "left_rows_outside", "left_rows_wrap", "right_rows", "right_rows_outside",
          "right_rows_wrap", "two_octaves_away", "bucket_0", "bucket_1_32", "bucket_33_64", "bucket_65_96",
          "bucket_97_up", "bucket_max", "iniu_negative", "endu_past_cols", "sad_denominator_zero", "matched")


def _row_run(w: int, h: int, r: int, c0: int, n: int) -> tuple[bool, bool]:
    """Pixels (r, c0 .. c0 + n - 1) of a level's sheared view, whose row r starts r * w bytes after the level's
    first pixel inside the (w + 2 EDGE)-wide padded level: (the run leaves the level, it wraps into the next
    padded row)."""
    pw = w + 2 * EDGE
    f = EDGE * pw + EDGE + r * w + c0
    pr, pc = divmod(f, pw)
    inside = EDGE <= pr < EDGE + h and pc >= EDGE and pc + n <= EDGE + w
    return not inside, pc + n > pw


def census(left_ref, right_ref, bf: float, fx: float) -> tuple[dict, list]:
    """(counts, one label per left keypoint).  The left keypoints are walked in order and each right keypoint
    whose row band holds the left one's row is a candidate, as the reference walks them; float32 where the
    reference's NumPy chain is float32."""
    f32 = np.float32
    kl, kr = left_ref.kps, right_ref.kps
    scale = [float(v) for v in left_ref.tables["scale"]]
    inv_scale = [float(v) for v in left_ref.tables["inv_scale"]]
    c = dict.fromkeys(COUNTS, 0)
    labels = []
    yr = [float(v) for v in kr["y"]]
    band = [(math.floor(y - 2.0 * scale[int(o)]), math.ceil(y + 2.0 * scale[int(o)])) for y, o in zip(yr, kr["octave"])]
    max_d = f32(bf) / (f32(bf) / f32(fx))
    for i in range(len(kl)):
        u_l, v_l, oct_l = f32(kl["x"][i]), float(kl["y"][i]), int(kl["octave"][i])
        bucket = [j for j, (lo, hi) in enumerate(band) if lo <= int(v_l) <= hi]
        n = len(bucket)
        c["bucket_max"] = max(c["bucket_max"], n)
        c["bucket_0" if n == 0 else "bucket_1_32" if n <= 32 else "bucket_33_64" if n <= 64 else
          "bucket_65_96" if n <= 96 else "bucket_97_up"] += 1
        if n == 0:
            labels.append(EMPTY_BUCKET)
            continue
        min_u = u_l - max_d
        best, best_j, n_best = 10 ** 9, -1, 0
        dist = stereo_oracle.hamming_rows(left_ref.desc[i], right_ref.desc[bucket])
        for j, d in zip(bucket, (int(v) for v in dist)):
            if abs(int(kr["octave"][j]) - oct_l) > 1:
                c["two_octaves_away"] += 1
                continue
            u_r = f32(kr["x"][j])
            c["ur_eq_minu"] += int(u_r == min_u)
            if not (min_u <= u_r <= u_l):
                continue
            if d < best:
                best, best_j, n_best = d, j, 1
            elif d == best:
                n_best += 1
        if best_j < 0:
            labels.append(NO_CANDIDATE)
            continue
        c["best_74"] += int(best == 74)
        c["best_75"] += int(best == 75)
        if best >= 75:
            labels.append(FAR_DESCRIPTOR)
            continue
        c["distance_ties_below_75"] += int(n_best > 1)
        # the 11 x 11 patch around the left keypoint against the same patch at 11 shifts in the right level
        lvl_l, lvl_r = left_ref.sheared[oct_l], right_ref.sheared[oct_l]
        lh, lw = lvl_l.shape
        su_l, sv_l = round(float(u_l) * inv_scale[oct_l]), round(v_l * inv_scale[oct_l])
        su_r = round(float(kr["x"][best_j]) * inv_scale[oct_l])
        if su_r < 0 or su_r + 11 >= lw:  # iniu = su_r + L - w, endu = su_r + L + w + 1 with L = w = 5
            c["iniu_negative" if su_r < 0 else "endu_past_cols"] += 1
            labels.append(STRIP_LEAVES)
            continue
        c[f"refined_octave{oct_l}"] += 1
        for r in range(sv_l - 5, sv_l + 6):
            out, wrap = _row_run(lw, lh, r, su_l - 5, 11)
            c["left_rows"] += 1
            c["left_rows_outside"] += int(out)
            c["left_rows_wrap"] += int(wrap)
            out, wrap = _row_run(lw, lh, r, su_r - 10, 21)
            c["right_rows"] += 1
            c["right_rows_outside"] += int(out)
            c["right_rows_wrap"] += int(wrap)
        patch = lvl_l[sv_l - 5:sv_l + 6, su_l - 5:su_l + 6].astype(np.int64)
        patch = patch - patch[5, 5]
        sads = []
        for inc in range(-5, 6):
            win = lvl_r[sv_l - 5:sv_l + 6, su_r + inc - 5:su_r + inc + 6].astype(np.int64)
            sads.append(int(np.abs(patch - (win - win[5, 5])).sum()))
        k = sads.index(min(sads))  # the first minimum
        c["sad_min_ties"] += int(sads.count(sads[k]) > 1)
        if k in (0, 10):
            c["bestinc_minus_l" if k == 0 else "bestinc_plus_l"] += 1
            labels.append(MIN_AT_END)
            continue
        d1, d2, d3 = sads[k - 1], sads[k], sads[k + 1]
        if d1 + d3 - 2 * d2 == 0:
            c["sad_denominator_zero"] += 1
            labels.append(STEEP_PARABOLA)
            continue
        delta = f32(d1 - d3) / f32(2 * (d1 + d3 - 2 * d2))
        if delta < -1 or delta > 1:
            labels.append(STEEP_PARABOLA)
            continue
        best_u = f32(scale[oct_l]) * (f32(su_r + k - 5) + delta)
        disparity = u_l - best_u
        if disparity < 0:
            c["disparity_negative"] += 1
            labels.append(DISPARITY_OUT)
        elif disparity >= max_d:
            c["disparity_ge_maxd"] += 1
            labels.append(DISPARITY_OUT)
        else:
            c["accepted_within_1px_of_maxd"] += int(max_d - disparity <= 1)
            if disparity == 0:
                c["disparity_zero"] += 1
                c["disparity_zero_octave0"] += int(oct_l == 0)
                labels.append(ZERO)
            else:
                labels.append(MATCH)
            c["matched"] += 1
    return c, labels


@functools.lru_cache(maxsize=None)
def census_of(case_id: str):
    c = next(c for c in ALL_CASES if c.id == case_id)
    return census(image_ref(c.group, 0), image_ref(c.group, 1), c.bf, c.fx)
