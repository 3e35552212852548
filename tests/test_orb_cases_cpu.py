"""CPU pre-conditions of tests/test_gpu_orb_edges.py and the definition-level check of the oracle's last stage.

  * the fixtures of orb_cases.py keep their promises on the oracle's output: every placement, both pair halves,
    every angle class, sector and steering extreme (no class is waived);
  * orb_definition.py (umax from the formula, moments over the disc, fastAtan2 from OpenCV's definition, the host
    libm's cosf / sinf, sample coordinates rounded once from an exact sum) reproduces the oracle's angle bits and
    all 32 descriptor bytes of every keypoint of every fixture image and of a noise image;
  * the other reading of the sample coordinate (product rounded before the sum) does not;
  * known angles, and every angle against float64 atan2 within the measured error bound of cv::fastAtan2.
"""
import functools
import math

import numpy as np
import pytest

import orb_cases as K
import orb_definition as D
from oracle import oracle as O

# The largest error of the oracle's fast_atan2 against float64 atan2 over a dense sweep (ratios min / max of
# 0 .. 1 in steps of 2.5e-6 at four magnitudes, both argument orders, plus 200 000 random integer moments in all
# octants) is 0.009546 degrees, just below a ratio of 1 (the diagonals); rounded up to the next 0.005 degrees.
# test_fast_atan2_error_bound repeats a coarser sweep.  Not derived from the kernel.
ATAN2_TOL_DEG = 0.010

needs_fma_libm = pytest.mark.skipif(not D.host_libm_is_the_fma_variant(),
                                    reason="the oracle's cosf / sinf replicate glibc's x86-64 FMA variant only")


def _sets() -> dict:
    return {"placement": K.placement_set(), "orientation": K.orientation_set()}


def _ref(case: K.Case) -> K.Ref:
    return K.ref(case.name)


@functools.lru_cache(maxsize=None)
def _restated(case_name: str, fused: bool = True):
    """orb_definition's (angles, descriptors, reach) of every keypoint the oracle keeps in a case, computed once."""
    case = next(c for c in K.placement_set() + K.orientation_set() + (K.noise_case(),) if c.name == case_name)
    ref = _ref(case)
    angles = np.zeros(len(ref.kps), np.float32)
    desc = np.zeros((len(ref.kps), 32), np.uint8)
    reach = D.new_reach()
    for l in range(case.nlevels):
        m = np.nonzero(ref.level == l)[0]
        a, d = D.describe_level(ref.pyramid[l], list(zip(ref.cx[m], ref.cy[m])), fused, reach)
        angles[m], desc[m] = a, d
    return angles, desc, reach


def _moments(case: K.Case):
    ref = _ref(case)
    return [D.moments(ref.pyramid[l], int(x), int(y)) for l, x, y in zip(ref.level, ref.cx, ref.cy)]


# ---- the fixtures keep their promises ---------------------------------------------------------------------------
def test_every_promised_keypoint_is_kept():
    n = 0
    for cases in _sets().values():
        for c in cases:
            kept = K.ref(c.name).index()
            for p in c.promises:
                assert (p.level, p.cx, p.cy) in kept, (c.name, p)
                n += 1
            assert c.image.shape == (K.H, K.W) and c.image.dtype == np.uint8
    assert (K.W * K.H) % 4 == 3
    assert n > 200


def test_placement_set_covers_every_staging_class():
    """Level 0: the full product of the column edges {19, 24, 25, Lw-23, Lw-22, Lw-20} and the row edges {19, 20,
    21, Lh-22, Lh-21, Lh-20}, and the alignment runs; level 1: the listed corners.  The edges are the decision
    points themselves: 24 | 25 and Lw-23 | Lw-22 switch the columns' path, 20 | 21 and Lh-22 | Lh-21 the rows'."""
    promised = {(p.level, p.cx, p.cy) for c in K.placement_set() for p in c.promises}
    lw, lh = K.W, K.H
    for cx in (19, 24, 25, lw - 23, lw - 22, lw - 20):
        for cy in (19, 20, 21, lh - 22, lh - 21, lh - 20):
            assert (0, cx, cy) in promised, (cx, cy)
    for cy in (20, 21, lh - 22, lh - 21):
        for cx in (25, 26, 27, 28, lw - 26, lw - 25, lw - 24, lw - 23):
            assert (0, cx, cy) in promised, (cx, cy)
    assert [K.staging_class(lw, lh, cx, 40).split(", ")[0] for cx in (19, 24, 25, lw - 23, lw - 22, lw - 20)] == \
        ["byte columns", "byte columns", "dword columns", "dword columns", "byte columns", "byte columns"]
    assert [K.staging_class(lw, lh, 40, cy).split(", ")[1] for cy in (20, 21, lh - 22, lh - 21)] == \
        ["reflected rows", "rows inside", "rows inside", "reflected rows"]
    l1w, l1h = K.level_sizes(K.PLACEMENT_LEVELS)[1]
    assert (l1w, l1h) == (109, 81)
    for t in [(19, 19), (24, 20), (25, 21), (l1w - 23, l1h - 22), (l1w - 22, l1h - 21), (l1w - 20, l1h - 20),
              (l1w - 26, l1h - 22), (l1w - 25, l1h - 22), (l1w - 24, l1h - 22)]:
        assert (1,) + t in promised, t
        assert t in K.level1_targets()


def test_alignment_runs_reach_every_misalignment_and_the_buffers_end():
    """The dword path loads from the dword at or below byte a = (cy - 21 + r) W + cx - 25 + bias of window row r and
    shifts by a & 3.  With the biases 0 .. 3 of a batch's image slots (W H = 3 mod 4) each run of four columns gives
    every shift for every bias; and the last row's loads (52 bytes from the aligned start) of the run at the
    bottom-right corner, row Lh - 22, end within 4 bytes of the bound W H + bias for every residue of the bound."""
    w, h = K.W, K.H
    residues = set()
    for bias in range(4):
        for run in (range(25, 29), range(w - 26, w - 22)):
            for cy in (21, h - 22):
                assert {((cy - 21) * w + cx - 25 + bias) & 3 for cx in run} == {0, 1, 2, 3}
        bound = w * h + bias
        residues.add(bound % 4)
        for cx in range(w - 26, w - 22):
            a = (h - 22 - 21 + 42) * w + cx - 25 + bias
            end = (a & ~3) + 52
            assert abs(end - bound) <= 4, (bias, cx, end, bound)
        assert any(((h - 1) * w + cx - 25 + bias & ~3) + 52 > bound for cx in range(w - 26, w - 22))  # and past it
    assert residues == {0, 1, 2, 3}


def test_reflected_pixels_decide_descriptor_bits_on_every_side():
    """The four searched cases: extending the level by its edge pixel or by zeros instead of reflect-101 along the
    axis changes the promised keypoint's descriptor, so a kernel that reflects wrongly on that side fails on it.
    Of the other promised border keypoints only some depend on the reflected pixels (a sample must land within 3 px
    of the border and tip a comparison): counted, and at least the searched four."""
    for side, cx, cy, _, _ in K.REFLECTION:
        r = K.ref(f"reflection {side}")
        dep = K.border_dependence(r, r.index()[(0, cx, cy)])
        assert dep and all(dep.values()), (side, dep)
        assert set(dep) == ({"columns"} if side in ("left", "right") else {"rows"})
    dependent = total = 0
    for c in K.placement_set():
        r = K.ref(c.name)
        for p in c.promises:
            dep = K.border_dependence(r, r.index()[(p.level, p.cx, p.cy)])
            total += len(dep)
            dependent += sum(dep.values())
    assert dependent >= 4 and total >= 60, (dependent, total)


def test_extreme_dword_placements_are_both_halves_of_a_pair():
    """({25, Lw-23} x {21, Lh-22}) each at an even and at an odd position of level 0's output order: A and B of a
    wave's keypoint pair (a wave starts at an even position in every describe shape)."""
    assert K.EXTREME_DWORD == [(25, 21), (25, K.H - 22), (K.W - 23, 21), (K.W - 23, K.H - 22)]
    for cx, cy in K.EXTREME_DWORD:
        parities = set()
        for c in K.placement_set():
            if any((p.level, p.cx, p.cy) == (0, cx, cy) for p in c.promises):
                r = K.ref(c.name)
                assert np.all(np.diff(r.level) >= 0)  # level-major output
                parities.add(int(r.pos[r.index()[(0, cx, cy)]]) % 2)
        assert parities == {0, 1}, (cx, cy, parities)


def _promised_angles() -> dict:
    """label -> the oracle's angles of the orientation set's centres with that label."""
    out = {}
    for c in K.orientation_set():
        r = K.ref(c.name)
        idx = r.index()
        for p in c.promises:
            out.setdefault(p.label, []).append(np.float32(r.kps["angle"][idx[(p.level, p.cx, p.cy)]]))
    return out


def test_orientation_set_holds_every_angle_class():
    by_label = _promised_angles()
    for lab in ["zero moment"] + [f"axis {s}" for s in ("+x", "+y", "-x", "-y")] + \
            [f"diagonal ({dx}, {dy})" for dx, dy in ((8, 8), (-8, 8), (-8, -8), (8, -8))]:
        assert len(by_label.get(lab, [])) == 1, lab
    # the centres' moments are what the groups were built for: zero, an axis, |m01| = |m10|
    groups = K.orientation_groups()
    for c in K.orientation_set():
        r = K.ref(c.name)
        for p in c.promises:
            m = D.moments(r.pyramid[0], p.cx, p.cy)
            assert m == K.group_moments(groups[(c.name, p.cx, p.cy)]), (c.name, p)
            if p.label == "zero moment":
                assert m == (0, 0)
            if p.label.startswith("axis"):
                assert (m[0] == 0) != (m[1] == 0)
            if p.label.startswith("diagonal"):
                assert abs(m[0]) == abs(m[1]) > 0
    # both sides of every multiple of 45 degrees, within 2 degrees
    for k in range(8):
        for side, word in ((-1, "below"), (1, "above")):
            (a,) = by_label[f"octant boundary {45 * k} {word}"]
            off = (float(a) - 45.0 * k + 180.0) % 360.0 - 180.0
            assert 0.0 < side * off < 2.0, (k, word, a)


def test_orientation_set_ratio_variety():
    pairs, sectors = set(), set()
    for c in K.orientation_set():
        r = K.ref(c.name)
        pairs |= set(_moments(c))
        sectors |= set((r.kps["angle"] // 15).astype(int).tolist())
    assert len(pairs) >= 200, len(pairs)
    assert sectors >= set(range(24)), sorted(set(range(24)) - sectors)


@needs_fma_libm
def test_orientation_set_steers_to_both_ends_of_the_tile():
    """Sampled rows and columns of -18 and +18 (the s_h tile's reach) both occur, as orb_definition computes them."""
    rows, cols = set(), set()
    for c in K.orientation_set():
        reach = _restated(c.name)[2]
        rows |= reach["rows"]
        cols |= reach["cols"]
    assert min(rows) == -18 and max(rows) == 18, (min(rows), max(rows))
    assert min(cols) == -18 and max(cols) == 18, (min(cols), max(cols))


# ---- the restatement equals the oracle --------------------------------------------------------------------------
def test_umax_from_the_formula():
    t = O.OracleExtractor(**K.params(1)).tables()
    assert list(D.umax_table()) == t["umax"].tolist()


def test_fast_atan2_definition_equals_the_oracle():
    """Bit for bit over zero moments, equal magnitudes, the axes and random integer moments."""
    L = O.lib()
    rng = np.random.default_rng(11)
    cases = [(y, x) for y in (-7, -1, 0, 1, 7, 1550) for x in (-7, -1, 0, 1, 7, 1550)]
    cases += rng.integers(-3_000_000, 3_000_000, (3000, 2)).tolist()
    cases += [(s * v, t * v) for v in rng.integers(1, 3_000_000, 200).tolist() for s in (-1, 1) for t in (-1, 1)]
    for y, x in cases:
        got, exp = D.fast_atan2(y, x), np.float32(L.oracle_fast_atan2(float(y), float(x)))
        assert got.view(np.uint32) == exp.view(np.uint32), (y, x, got, exp)


@needs_fma_libm
@pytest.mark.parametrize("which", ["placement", "orientation", "noise"])
def test_restatement_reproduces_the_oracle(which):
    """Angle (float32 bits) and all 32 descriptor bytes of every keypoint of every fixture image and of the noise
    image."""
    cases = (K.noise_case(),) if which == "noise" else _sets()[which]
    n = 0
    for c in cases:
        ref = _ref(c)
        angles, desc, _ = _restated(c.name)
        for i in range(len(ref.kps)):
            where = K.describe_keypoint(c, ref, i) if which != "noise" else (c.name, i)
            assert angles[i].view(np.uint32) == ref.kps["angle"][i].view(np.uint32), where
            assert desc[i].tobytes() == ref.desc[i].tobytes(), where
        n += len(ref.kps)
    assert n >= {"noise": 290, "placement": 90, "orientation": 300}[which], n


@needs_fma_libm
def test_unfused_reading_differs_from_the_oracle():
    """Rounding px * b before the sum gives another descriptor for at least one keypoint of the noise image (its
    seed was searched for that, see orb_cases.noise_case), so the comparison above can tell the two readings of
    ORBextractor.cpp:121-125 apart; the fused one is the oracle's."""
    ref = K.ref("noise")
    _, fused, _ = _restated("noise")
    _, unfused, _ = _restated("noise", False)
    differ = [i for i in range(len(ref.kps)) if unfused[i].tobytes() != ref.desc[i].tobytes()]
    assert len(differ) >= 1
    assert all(fused[i].tobytes() == ref.desc[i].tobytes() for i in differ)


# ---- angles -------------------------------------------------------------------------------------------------------
def test_known_angles():
    by_label = _promised_angles()
    for lab, exp in (("zero moment", 0.0), ("axis +x", 0.0), ("axis +y", 90.0), ("axis -x", 180.0), ("axis -y", 270.0)):
        (a,) = by_label[lab]
        assert a.view(np.uint32) == np.float32(exp).view(np.uint32), (lab, a)


def test_fast_atan2_error_bound():
    L = O.lib()
    worst = 0.0
    for den in (1 << 20, 3_000_000):
        for num in range(0, den + 1, den // 20_000):
            for y, x in ((num, den), (den, num), (-num, den), (den, -num), (-den, -num), (num, -den)):
                e = abs((L.oracle_fast_atan2(float(y), float(x)) - math.degrees(math.atan2(y, x)) + 180) % 360 - 180)
                worst = max(worst, e)
    assert 0.009 < worst <= ATAN2_TOL_DEG, worst


def test_every_fixture_angle_is_close_to_atan2():
    n = 0
    for c in K.placement_set() + K.orientation_set() + (K.noise_case(),):
        ref = _ref(c)
        for i, (m01, m10) in enumerate(_moments(c)):
            exact = math.degrees(math.atan2(m01, m10)) % 360.0
            err = abs((float(ref.kps["angle"][i]) - exact + 180.0) % 360.0 - 180.0)
            assert err <= ATAN2_TOL_DEG, (c.name, i, m01, m10, ref.kps["angle"][i], exact)
            n += 1
    assert n > 700
