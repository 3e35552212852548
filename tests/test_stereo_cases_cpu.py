"""The inputs of tests/test_gpu_stereo_edges.py reach the gates they are built for (oracle, restatement and the
reference's goldens only, no GPU): for every case the restatement equals the golden, the census derived from the
inputs equals the stored one and its labels imply the golden's statuses; over the set every gate of
Frame.compute_stereo_matches decides often enough that a kernel wrong at that gate cannot pass.

The minimum counts are conditions on the inputs, about half of what seed 1 yields (the measured figure stands
beside each); they are not measurements of the code under test."""
import hashlib

import numpy as np
import pytest

import stereo_cases as SC

CASE_IDS = [c.id for c in SC.ALL_CASES]


def _case(cid):
    return next(c for c in SC.ALL_CASES if c.id == cid)


def _count(cid, key):
    return SC.golden_of(_case(cid))["census"][key]


def test_case_list():
    assert len(SC.CASES) == len(SC.PAIRS) * len(SC.FXS) == 50 and len(SC.LONG_CASES) == 2
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    # an integer fx equal to the shift, and the half-integers on either side
    assert SC.FXS[:3] == (SC.SHIFT - 0.5, float(SC.SHIFT), SC.SHIFT + 0.5)
    for fx in SC.FXS:  # maxD = bf / (bf / fx) in float32 is fx itself
        assert np.float32(SC.BF) / (np.float32(SC.BF) / np.float32(fx)) == np.float32(fx)


@pytest.mark.parametrize("group", SC.GROUPS)
def test_inputs_are_the_goldens_inputs(group):
    g = SC.load_golden(group)
    for side, name in ((0, "left"), (1, "right")):
        ref = SC.image_ref(group, side)
        assert hashlib.sha256(ref.image.tobytes()).hexdigest() == str(g[f"{name}_sha"])
        assert hashlib.sha256(ref.kps.tobytes()).hexdigest() == str(g[f"kps_{name}_sha"])
        assert hashlib.sha256(ref.desc.tobytes()).hexdigest() == str(g[f"desc_{name}_sha"])


@pytest.mark.parametrize("cid", CASE_IDS)
def test_restatement_and_census_equal_the_golden(cid):
    case = _case(cid)
    g = SC.golden_of(case)
    status, u_right, depth, match_r = SC.restated(cid)
    assert np.array_equal(status, g["status"])
    assert np.array_equal(u_right, g["u_right"]) and np.array_equal(depth, g["depth"])
    assert np.array_equal(match_r >= 0, status > 0)
    counts, labels = SC.census_of(cid)
    assert counts == g["census"]
    assert [SC.STATUS_OF_LABEL.get(x, 0) for x in labels] == g["status"].tolist()
    assert counts["matched"] == int((g["status"] > 0).sum())
    assert counts["disparity_zero"] == int((g["status"] == 2).sum())
    # asserted zero: the reference's two strip conditions never hold (keypoints stay 19 px inside their level),
    # and no parabola has a zero denominator
    assert counts["iniu_negative"] == 0 and counts["endu_past_cols"] == 0 and counts["sad_denominator_zero"] == 0


# (case, census row, minimum, measured with seed 1)
REACHED = [
    ("noise3-fx3", "ur_eq_minu", 43, 86), ("coarse3-fx3", "ur_eq_minu", 44, 89),
    ("noise3-fx3", "disparity_ge_maxd", 24, 49), ("coarse3-fx3", "disparity_ge_maxd", 29, 58),
    ("noise3-fx3", "accepted_within_1px_of_maxd", 27, 54), ("coarse3-fx3", "accepted_within_1px_of_maxd", 28, 56),
    ("noise3-fx100", "best_74", 2, 3), ("noise3-fx100", "best_75", 1, 2),
    ("noisy40-fx100", "best_74", 2, 4), ("noisy70-fx100", "best_74", 3, 5), ("noisy70-fx100", "best_75", 1, 2),
    ("noise3_n1000-fx100", "best_75", 5, 9),
    ("lattice_same-fx100", "distance_ties_below_75", 56, 112), ("coarse3-fx100", "distance_ties_below_75", 1, 1),
    ("lattice_same-fx100", "sad_min_ties", 47, 94),
    ("noise3-fx100", "bestinc_minus_l", 2, 3), ("noise3-fx100", "bestinc_plus_l", 4, 8),
    ("noise3-fx100", "disparity_negative", 7, 14), ("noise_same-fx100", "disparity_negative", 76, 153),
    ("binary_same-fx100", "disparity_zero", 4, 7), ("lattice_same-fx100", "disparity_zero", 6, 11),
    ("lattice_same-fx3", "disparity_zero", 10, 20),
    ("noise3-fx100", "refined_octave0", 41, 82), ("noise3-fx100", "refined_octave1", 13, 26),
    ("noise3-fx100", "refined_octave2", 18, 36),
    ("noise3-fx100", "left_rows_wrap", 49, 98), ("noise3-fx100", "right_rows_wrap", 102, 205),
    ("noise3-fx100", "two_octaves_away", 1032, 2065), ("natural-fx100", "two_octaves_away", 180, 359),
    ("noise3_n1000-fx100", "bucket_65_96", 250, 500), ("noise3_n1000-fx100", "bucket_97_up", 108, 217),
    ("noise3_n1000-fx3", "bucket_65_96", 250, 500), ("noise3_n1000-fx3", "bucket_97_up", 108, 217),
    ("noise3_n1000-fx3", "ur_eq_minu", 225, 450), ("noise3_n1000-fx3", "disparity_ge_maxd", 112, 225),
    ("sparse_right-fx100", "bucket_0", 61, 122), ("sparse_right-fx100", "matched", 25, 50),
    ("sparse_right-fx3", "bucket_0", 61, 122), ("sparse_right-fx3", "matched", 10, 19),
]


@pytest.mark.parametrize("cid,key,minimum,measured", REACHED, ids=[f"{c}-{k}" for c, k, _, _ in REACHED])
def test_gate_is_reached(cid, key, minimum, measured):
    assert minimum > 0 and 2 * minimum + 1 >= measured
    assert _count(cid, key) >= minimum, (cid, key, _count(cid, key))


def test_issue_floors():
    """The floors that hold whatever the seed gives."""
    for pair in ("noise3", "coarse3"):
        assert _count(f"{pair}-fx3", "ur_eq_minu") >= 30
        assert _count(f"{pair}-fx2.5", "ur_eq_minu") == 0 and _count(f"{pair}-fx3.5", "ur_eq_minu") == 0
    wide = [c.id for c in SC.ALL_CASES if c.fx == 100.0]
    assert sum(_count(c, "best_74") for c in wide) >= 8   # measured 16
    assert sum(_count(c, "best_75") for c in wide) >= 8   # measured 16
    assert min(sum(_count(c, k) for c in wide) for k in ("best_74", "best_75")) >= 3
    for cid in ("noise3_n1000-fx3", "noise3_n1000-fx100"):
        assert _count(cid, "bucket_65_96") >= 100 and _count(cid, "bucket_97_up") >= 100
        assert _count(cid, "bucket_max") >= 97
    assert _count("sparse_right-fx100", "bucket_0") >= 50 and _count("sparse_right-fx100", "matched") > 0
    # every zero disparity is found at octave 0
    for c in SC.ALL_CASES:
        assert _count(c.id, "disparity_zero") == _count(c.id, "disparity_zero_octave0")
    # the nfeatures = 300 handle of the dense pairs never needs the search's third step, the other one does
    assert max(_count(f"{p}-fx100", "bucket_max") for p in SC.PAIRS if p != "sparse_right") <= 64
    assert _count("sparse_right-fx100", "bucket_65_96") >= 33  # measured 66


def test_window_rows_leave_the_level():
    """About 30 % of the left window rows and 38 % of the right ones leave the level or wrap in the sheared view
    (the lane-parallel border gather of the kernel); at least half of that."""
    c = SC.golden_of(_case("noise3-fx100"))["census"]
    assert c["left_rows_outside"] >= 0.15 * c["left_rows"] and c["left_rows"] >= 11 * 72
    assert c["right_rows_outside"] >= 0.19 * c["right_rows"]


@pytest.mark.parametrize("h", SC.TALL_HEIGHTS)
def test_tall_geometry_is_accepted_and_matches(h):
    """879 x 480 and 880 x 480 are accepted by the oracle (OracleExtractor raises where DistributeOctTree
    refuses), the two pairs differ and both match."""
    refs = [SC.tall_pair(h, k) for k in range(len(SC.TALL_SEEDS))]
    assert refs[0][0].kps.tobytes() != refs[1][0].kps.tobytes()
    for left, right, (status, _, _, match_r) in refs:
        assert left.image.shape == (h, SC.TALL_W)
        assert len(left.kps) >= 300 and len(right.kps) >= 300       # measured about 600
        assert int((status == 1).sum()) >= 120                      # measured about 240
        assert set(np.unique(left.kps["octave"])) == {0, 1, 2}
        # keypoints in the last rows: the row counters up to H - 1 are used
        assert int(left.kps["y"].max()) >= h - 25
