"""detect_lane_cases.py on the CPU: every image gives its target cell the window, the queue lengths and the outcome
the case states (numpy restatement of k_detect's pre-test bound, exact M and NMS, tools/detect_queue_stats.py), the
restatement's candidates equal the oracle's row for row, and every class the kernel's lane decisions need has a
case.  tests/test_gpu_detect_lanes.py runs the same images through the kernel."""
import numpy as np
import pytest

import detect_lane_cases as K

IDS = [c.name for c in K.CASES]

REQUIRED = (
    "empty half at y0 = 0", "live half at y0 = 0", "empty half at y0 = 16", "live half at y0 = 16",
    "empty half at y0 = 32", "live half at y0 = 32", "ROI above 48 rows", "generic pre-test, empty half",
    "generic pre-test, live half",
    "|A| mod 64 = 1", "|A| mod 64 = 63", "|A| mod 64 = 0", "|A| > 64",
    "|B| < free lanes", "|B| = free lanes", "|B| = free lanes + 1", "|B| - free lanes = 64",
    "no fallback, carried", "row-end pair carried", "A in the first half", "A in the second half",
)


def test_names_are_unique_and_every_class_has_a_case():
    assert len(set(IDS)) == len(IDS)
    assert set(REQUIRED) <= set(K.CLASSES), set(REQUIRED) - set(K.CLASSES)
    assert {K.by_name(f"wh {n}").expect["wh"] for n in (8, 9, 24, 25, 40, 41)} == {8, 9, 24, 25, 40, 41}


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_target_cell_is_what_the_case_states(case):
    r = dict(K.counts(case)[case.cell])
    r["a_halves"] = [int(h) for h in r["a_halves"]]
    got = {k: r[k] for k in case.expect}
    assert got == case.expect, (case.name, r)
    assert not any(c["collide"] for c in K.counts(case)), "the cases stay on the two-queue path"
    assert r["A"] <= r["B"] and r["kb"] == (0 if r["A"] == 0 else min(-r["A"] % 64, r["B"]))


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_restatement_equals_the_oracle(case):
    """The exact M, the NMS and the fallback of the restatement against the oracle's FAST cells: the fallback
    outcome of every cell is the oracle's."""
    cand = [tuple(r) for r in K.candidates(case).tolist()]
    assert cand == K.model_candidates(case)
    assert len(cand) > 0


def test_the_class_predicates():
    """What the classes mean, on the target cell's counts."""
    def t(name):
        c = K.by_name(name)
        return K.counts(c)[c.cell]
    free = lambda r: -r["A"] % 64
    for name, rem in (("A 1, B 5", 1), ("A 63", 63), ("A 64", 0), ("A 70", 6)):
        r = t(name)
        assert r["A"] % 64 == rem and r["fallback"], name
    assert t("A 70")["A"] > 64 and t("A 70")["kb"] == 58                    # only the last step carries
    assert t("A 64")["kb"] == 0 and t("A 64")["carry_steps"] == 0           # no free lane
    r = t("A 1, B 5")
    assert 0 < r["B"] < free(r) and r["b_steps"] == 0                       # B's M stage has no step left
    r = t("A 1, B 63")
    assert r["B"] == free(r) and r["b_steps"] == 0
    r = t("A 1, B 64")
    assert r["B"] == free(r) + 1 and r["b_steps"] == 1
    r = t("A 1, B 127")
    assert r["B"] - free(r) == 64 and r["b_steps"] == 1
    r = t("iniTh corner, B carried")
    assert not r["fallback"] and r["kb"] == r["B"] - 0 > 1
    assert t("A 1, B 5")["a_halves"][:2] == [True, False] and t("second half only")["a_halves"][:2] == [False, True]
    # 16 row slots only above 48 ROI rows: a window of 41 rows (ROI 47) still stages from 12
    assert t("wh 41")["wh"] + 6 <= 48 < t("wh 44, 16 row slots")["wh"] + 6
    for name in ("9 quads per row, odd halves", "9 quads per row, even halves"):
        assert t(name)["qrow"] > 8 and t(name)["A"] > 64 and t(name)["kb"] > 0


def test_row_end_pair_is_among_the_carried_entries():
    """Odd width: the window's last pair of row 2 (its second pixel outside the window, and the stronger corner) is
    one of the first kb entries of B, and the pixel inside is a minTh corner the cell keeps."""
    case = K.by_name("odd width, row end carried")
    D = K.model()
    M, bound = D.maps(K.image(case))
    cell = K.grid(case.size)[case.cell]
    r = K.counts(case)[case.cell]
    assert r["ww"] % 2 == 1
    pm, pb = D.pair_maps(M, bound, cell)
    order = [(y, p) for y, p in zip(*np.nonzero(pb > K.MIN))]               # B, row-major
    last = (r["ww"] - 1) // 2
    assert (2, last) in order[:r["kb"]]
    x0, y0 = cell[0] + 3, cell[1] + 3
    inside, outside = M[y0 + 2, x0 + r["ww"] - 1], M[y0 + 2, x0 + r["ww"]]
    assert K.MIN < inside < outside <= K.INI
    assert (int(x0 + r["ww"] - 1 - 16), int(y0 + 2 - 16), int(inside - 1)) in [tuple(c) for c in K.candidates(case).tolist()]
