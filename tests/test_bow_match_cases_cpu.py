"""Every k_bow_match case contains what it is for (CPU only: the array oracle runs the cases), so the GPU
comparison in tests/test_gpu_bow_match.py cannot pass vacuously."""
import numpy as np
import pytest

import bow_match_cases as BC
import bow_match_oracle as O

CASES = BC.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_holds_its_claim(case):
    res = BC.oracle(case)
    case["check"](res)
    for (a, b), (m12, m21, bin12, hist, n_raw) in zip(case["pairs"], res):
        assert len(m12) == len(case["frames"][a]["desc"]) and len(m21) == len(case["frames"][b]["desc"])
        assert int((m12 >= 0).sum()) == int((m21 >= 0).sum()) == n_raw == int(hist.sum())
        assert np.array_equal(bin12 >= 0, m12 >= 0)
        # the rotation cut condition: only the case built to break it does
        assert O.cut_is_stable(hist) == case["stable_cut"]


def test_case_list_covers_the_boundaries():
    names = {c["name"] for c in CASES}
    for L in (0, 1, BC.CHUNK - 1, BC.CHUNK, BC.CHUNK + 1, 2 * BC.CHUNK - 1, 2 * BC.CHUNK, 2 * BC.CHUNK + 1):
        assert f"run2_{L}" in names
    for L in (0, 1, 40):
        assert f"run1_{L}" in names
    assert sum(not c["stable_cut"] for c in CASES) == 1
    by = {c["name"]: c for c in CASES}
    assert len(by["sharing_waves_plus_one_pairs"]["pairs"]) == BC.WAVES + 1
    assert len(by["sharing_one_pair"]["pairs"]) == 1
    # more common nodes than waves in one pair, and frames of valid structure throughout
    assert len(by["nodes_many"]["frames"][0]["fv_node"]) > BC.WAVES
    for c in CASES:
        for f in c["frames"]:
            assert np.all(np.diff(f["fv_node"]) > 0) and np.all(np.diff(f["fv_end"]) >= 0)
            assert len(set(f["fv_idx"].tolist())) == len(f["fv_idx"]) <= len(f["desc"])


def test_multiply_and_divide_disagree_somewhere():
    """The reference multiplies by the double 1 / 30; a float32 angle pair exists for which dividing by 30 gives
    another bin, and the rotation case contains it."""
    sp = BC.half_bin_split()
    assert sp is not None
    rot = float(sp[0]) - float(sp[1])
    assert round(rot * (1.0 / 30)) != round(rot / 30)
    assert (float(sp[0]), float(sp[1])) in BC.rotation_pairs()


def test_reject_matches_the_reference_spelling():
    """reject() keeps exactly the bins np.argsort(counts)[::-1][:3] names."""
    hist = np.zeros(32, np.int32)
    hist[[2, 5, 7, 9]] = [4, 9, 1, 6]
    m12 = np.array([0, 1, 2, 3, -1], np.int32)
    m21 = np.array([0, 1, 2, 3], np.int32)
    bin12 = np.array([2, 5, 7, 9, -1], np.int8)
    r12, r21, n = O.reject(m12, m21, bin12, hist, 4)
    assert r12.tolist() == [0, 1, -1, 3, -1] and r21.tolist() == [0, 1, -1, 3] and n == 3
