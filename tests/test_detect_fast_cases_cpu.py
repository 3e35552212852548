"""detect_fast_cases.py on the CPU: the numpy restatement (tools/detect_queue_stats.py's maps, cv::FAST's score and
strict NMS per cell window, the iniTh -> minTh fallback) equals the oracle row for row on every case, every case has
the outcome it states, its candidate list changes under each mutant of the restatement it is named for, and every
class of decision has a case in every instantiation of k_detect that a geometry can reach.
tests/test_gpu_detect_fast.py runs the same images through the kernel."""
import numpy as np
import pytest

import detect_fast_cases as K

# class -> the mutant kinds one of which its cases must stand on (None: the outcome alone is asserted)
REQUIRED = {
    "arc": ("arc",), "arc, one threshold": ("arc",),
    "threshold sides": ("th_ge",), "iniTh side, no fallback": ("th_ge",), "iniTh side, fallback": ("th_ge",),
    "A pair without iniTh corner": None,
    "threshold ends (254, 254)": ("th_ge",), "threshold ends (255, 255)": ("th_ge",),
    "threshold ends (254, 253)": None, "threshold ends (255, 0)": ("nms_ge",), "threshold ends (0, 0)": ("nms_ge",),
    "threshold ends (20, 0)": ("nms_ge",), "threshold ends (7, 20)": None, "dark side, M = 255": None, "dark side, threshold 255": ("th_ge",),
    "NMS weaker": ("nms_dir",), "NMS tie, fallback": ("nms_ge", "fallback_pre"), "NMS tie, no fallback": ("nms_ge",),
    "cell boundary": ("nms_across", "window"), "cell boundary, odd width": ("nms_across",), "outer window edge": ("window",),
    "one-pass, nothing kept": None, "one-pass, minTh list copied": ("onepass_never",),
    "one-pass, minTh list discarded": ("onepass_always",),
}
ONLY_AT_48_12 = ("rem 1", "rem 2", "rem 3", "rem 4")    # the masks of the last quad do not depend on the instantiation


def _cand(case):
    return [tuple(r) for r in K.candidates(case).tolist()]


def test_geometries_reach_the_instantiations_and_both_pre_tests():
    assert set(K.GEO_A) == set(K.GEO_22) == set(K.REACHED) and len(K.REACHED) == 4
    for geo in (K.GEO_A, K.GEO_22):
        for inst, size in geo.items():
            g = K.geometry(size)
            assert g["inst"] == inst and g["accepted"], (size, g)
    assert all(K.geometry(s)["inst"] == (48, 12) for s in K.GEO_WIDTHS)
    assert all(K.geometry(s)["inst"] == inst and K.window(s, 0)[2] % 2 == 1 for inst, s in K.GEO_ODD_64.items())
    assert max(K.geometry(K.GEO_A[48, 12])["qrow"]) == 8 and K.geometry(K.GEO_A[64, 12])["qrow"] == [11]
    assert {K.geometry(s)["rem"][-1] for s in K.GEO_WIDTHS} == {1, 2, 3, 4}
    assert [K.window((102, 108), c)[:2] for c in (1, 2)] == [(54, 19), (19, 57)]
    # <96, 16>: no level whose cell grid the host accepts (ROIs of at most 59 x 64) has a ROI wider than 61 px
    assert set(K.INSTANTIATION_OUT_OF_REACH) == {(96, 16)}
    for w in range(33, 400):
        cs = K.grid((w, 80))
        if cs:
            rw = max(c[2] - c[0] for c in cs)
            assert rw <= 59 and K.detect_rp(rw) != 96, w
    assert K.detect_rp(59) == 64 and K.detect_rp(61) == 64 and K.detect_rp(62) == 96 and K.detect_rp(45) == 48
    assert K.geometry((90, 70))["inst"] == (64, 12)      # the widest single cell column stays below RP = 96


def test_names_are_unique():
    assert len(set(K.IDS)) == len(K.IDS)


def test_the_unmutated_m_map_is_the_tools():
    img = K.by_name("A (48, 12) image 0 th (20, 7)").img
    M = K.model().maps(img)[0]
    full = M.copy()
    for k in range(16):
        for bright in (True, False):
            part = K.m_map(img, (k, bright))
            assert (part <= M).all()
            full = np.minimum(full, part)
    assert (full < M).any() and np.array_equal(K.m_map(img), M)


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_restatement_equals_the_oracle_and_the_stated_outcome(case):
    cand = _cand(case)
    assert cand == K.restate(case.img, case.th)
    if case.expect is not None:
        assert tuple(sorted((x + 16, y + 16, r) for x, y, r in cand)) == case.expect


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_case_stands_on_its_decisions(case):
    base = K.restate(case.img, case.th)
    for mut in case.mutants:
        assert K.restate(case.img, case.th, mut) != base, (case.name, mut)
    kinds = {m[0] for m in case.mutants}
    for cl in case.classes:
        if cl in REQUIRED and REQUIRED[cl]:
            assert kinds & set(REQUIRED[cl]), (case.name, cl)


@pytest.mark.parametrize("case", [c for c in K.CASES if c.family == "A"], ids=[c.name for c in K.CASES if c.family == "A"])
def test_stamp_centres(case):
    """Every positive stamp's centre is a candidate with response 31 that arc k of its polarity alone carries; the
    arc of 8 is none."""
    cand = {(x + 16, y + 16): r for x, y, r in _cand(case)}
    for s in case.info["stamps"]:
        at = (s["X"], s["Y"])
        if s["neg"]:
            assert at not in cand, (case.name, s)
        else:
            assert cand.get(at) == 31, (case.name, s)
            if case.th == (K.L.INI, K.L.MIN):
                without = {(x + 16, y + 16) for x, y, _ in K.restate(case.img, case.th, ("arc", s["k"], s["bright"]))}
                other = {(x + 16, y + 16) for x, y, _ in K.restate(case.img, case.th, ("arc", s["k"], not s["bright"]))}
                assert at not in without and at in other, (case.name, s)


def test_every_stamp_in_every_instantiation():
    """Family A allows no gap: arc x polarity x pixel of the pair, and its negative, in each reachable instantiation and
    at each of the three threshold settings; stamps in the first and last row and column of a window."""
    for inst in K.REACHED:
        for th in ((20, 7), (20, 20), (7, 7)):
            stamps = [s for c in K.CASES if c.family == "A" and c.inst == inst and c.th == th for s in c.info["stamps"]]
            assert sorted((s["k"], s["bright"], s["parity"], s["neg"]) for s in stamps) == sorted(K.STAMPS), (inst, th)
            assert all(s["x"] % 2 == s["parity"] for s in stamps)
            pos = [s for s in stamps if not s["neg"]]
            for side in range(4):
                assert {s["bright"] for s in pos if s["edge"][side]} == {True, False}, (inst, side)


def test_nms_cases_cover_directions_pixels_and_neighbour_classes():
    for inst in K.REACHED:
        for scen in ("weaker", "tie, fallback", "tie, no fallback"):
            seen = {(c.info["parity"], d) for c in K.CASES
                    if c.family == "C" and c.inst == inst and f"NMS {scen}" in c.classes for d in c.info["dirs"]}
            assert seen == set(K.NMS_CLASS), (inst, scen)
    assert set(K.NMS_CLASS.values()) == {"inside the pair", "next pair in the row", "row above or below"}


def test_one_pass_cases_take_the_one_pass_path():
    for case in (c for c in K.CASES if c.family == "E"):
        r = K.counts(case)[0]
        assert r["collide"] and r["A"] + r["B"] > max(K.model().pair_cap(c) for c in K.grid(case.size)), case.name
        assert len(_cand(case)) == len(case.expect) <= 1
    for case in (c for c in K.CASES if c.family != "E" and c.th[1] < c.th[0]):
        assert not any(r["collide"] for r in K.counts(case)), case.name


def test_every_class_has_a_case_in_every_instantiation():
    have = {(cl, c.inst) for c in K.CASES for cl in c.classes}
    missing = [(cl, inst) for cl in REQUIRED for inst in K.REACHED if (cl, inst) not in have]
    assert not missing, missing
    assert all((cl, (48, 12)) in have for cl in ONLY_AT_48_12)
    assert {cl for c in K.CASES for cl in c.classes} <= set(REQUIRED) | set(ONLY_AT_48_12)
    # every mutant of the restatement is what some case stands on, in every instantiation
    for kind in K.MUTANT_CLASSES:
        for inst in K.REACHED:
            assert any(m[0] == kind for c in K.CASES if c.inst == inst for m in c.mutants), (kind, inst)
    assert len(K.INSTANTIATION_OUT_OF_REACH) <= 4 and all(len(v) > 20 for v in K.INSTANTIATION_OUT_OF_REACH.values())
