"""octree_cases.py on the CPU: every image yields exactly the candidate list it promises, the oracle's octree
equals the traced definition on it, the trace shows every class the case is named for, and every class of
octree_cases.CLASSES has a case.  tests/test_gpu_octree_edges.py runs the same set through the kernels."""
import numpy as np
import pytest

import octree_cases as K
import octree_definition as OD
from oracle import oracle as O

IDS = [c.name for c in K.CASES]


def test_case_names_are_unique_and_classes_exist():
    assert len(set(IDS)) == len(IDS)
    for c in K.CASES:
        assert c.classes, f"{c.name}: unclassified"
        assert set(c.classes) <= set(K.CLASSES), (c.name, set(c.classes) - set(K.CLASSES))


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_image_yields_the_placed_candidates(case):
    ex = O.OracleExtractor(**case.params)
    ex.extract(K.image(case))
    pyr = ex.pyramid()
    assert [lvl.shape[::-1] for lvl in pyr][-1] == case.level_size and pyr[0].shape[::-1] == case.size
    n_per = ex.tables()["n_per_level"]
    assert int(n_per[case.level]) == K.level_target(case)
    if case.level:
        assert len(O.level_candidates(ex.p, pyr[0])) == 0   # cells and no key
    else:
        assert n_per.tolist() == [case.N]
    cand = O.level_candidates(ex.p, pyr[case.level])
    assert [tuple(r) for r in cand.tolist()] == K.placed(case)
    xs, ys = cand[:, 0], cand[:, 1]
    i = K.info(case)
    assert xs.min() >= 3 and xs.max() <= i.sx - 4 and ys.min() >= 3 and ys.max() <= i.sy - 4


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_oracle_octree_equals_the_traced_definition(case):
    i = K.info(case)
    w, h = case.level_size
    got = O.octree(np.array(i.K, np.int32), K.BORDER, w - K.BORDER, K.BORDER, h - K.BORDER, i.N)
    assert [tuple(r) for r in got.tolist()] == i.kept
    assert OD.octree_py(i.K, K.BORDER, w - K.BORDER, K.BORDER, h - K.BORDER, i.N) == i.kept  # the trace changes nothing
    assert len(i.kept) <= K.kp_cap(i.n_ini, i.N) - 2
    assert len(i.tr.final) == len(i.kept) and len(i.tr.divided_depths) == len(i.tr.divided_boxes)
    assert sum(len(d) for d in i.tr.pass_depths) + sum(it.divided for it in i.tr.careful) == len(i.tr.divided_depths)
    assert 1 <= i.D0 <= i.D and max(f[0] for f in i.tr.final) <= i.D


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_trace_shows_the_case_s_classes(case):
    i = K.info(case)
    tr = i.tr
    seen = dict(form=i.form, N=i.N, K=len(i.K), D=i.D, D0=i.D0, passes=tr.full_passes, lengths=tr.pass_lengths,
                switch=tr.switch_tests, full_end=tr.full_end, careful_end=tr.careful_end,
                iterations=[(len(it.candidates), it.divided, it.length, it.runs[:4]) for it in tr.careful],
                depths=sorted(set(tr.divided_depths)), kept=len(i.kept))
    for name in case.classes:
        assert K.CLASSES[name](i), f"{case.name} does not reach {name!r}: {seen}"


def test_straddled_ties_would_catch_the_other_order():
    """For every case named for a straddled tie, dividing the oldest of the equal-size nodes first keeps another
    set; for the tie that lies wholly before the break it keeps the same set (the order at most)."""
    n = 0
    for case in K.CASES:
        i = K.info(case)
        for name in case.classes:
            if "straddles" in name:
                assert sorted(i.kept) != sorted(i.kept_reversed), case.name
                n += 1
            if "wholly before" in name:
                assert sorted(i.kept) == sorted(i.kept_reversed), case.name
                last = i.tr.careful[-1]
                assert any(r[1] + r[2] == last.divided and not r[3] for r in last.runs), case.name
                n += 1
    assert n >= 4


def test_the_two_pass_implementations_meet_at_508_and_509():
    a, b = K.by_name("F nfeatures 508"), K.by_name("F nfeatures 509")
    assert (a.N, b.N) == (508, 509) and K.dots_of(a) == K.dots_of(b) and len(K.dots_of(a)) == 3731
    ia, ib = K.info(a), K.info(b)
    assert (ia.max_ncap, ib.max_ncap) == (512, 513) and (ia.form, ib.form) == ("flat", "lds")
    assert len(ia.kept) == len(ib.kept) == 509


def test_key_table_pair():
    a, b = K.by_name("F key walk"), K.by_name("F key table")
    ia, ib = K.info(a), K.info(b)
    assert a.N == b.N and ia.max_ncap == ib.max_ncap
    assert len(ib.K) <= K.key_table_cap(ib.max_ncap) < len(ia.K)
    assert {d[:2] for d in K.dots_of(b)} < {d[:2] for d in K.dots_of(a)}


def test_every_class_has_a_case():
    claimed = {n for c in K.CASES for n in c.classes}
    missing = [n for n in K.CLASSES if n not in claimed]
    assert not missing, missing
    for name, why in K.LDS_OUT_OF_REACH.items():
        assert name in K.FORM_CLASSES and f"{name} [flat]" in claimed and why
    # and the forms: every case of groups A - C is in exactly the form its classes say
    for c in K.CASES:
        forms = {n[-6:] for n in c.classes if n.endswith("]")}
        assert len(forms) <= 1, c.name
