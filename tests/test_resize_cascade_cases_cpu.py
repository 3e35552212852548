"""The cases of tests/test_gpu_resize_cascade.py reach the decisions of k_resize_cascade and of its host rules
they are chosen for, by the restatement in tests/resize_cascade_cases.py (no GPU): without this a GPU comparison
could pass on inputs that never reach the code it is meant for.  The restated strip tables are checked for the
properties the kernel relies on."""
import numpy as np
import pytest

import resize_cascade_cases as K
import sweep_cases as S


def _strips(case) -> int:
    """The strip count a case runs with (an automatic one at the nominal CU count), 0 for the per-level launches."""
    h, w, nlevels, scale, simd, strips = case
    return K.chosen_strips(h, w, nlevels, scale, K.NOMINAL_CUS, 1) if strips == K.AUTO else strips


def _area_ties(case) -> set:
    """Parities of the quotients of the 2 x 2 sums that are 2 mod 4 in the scalar tail of an area level."""
    h, w, nlevels, scale, simd, _ = case
    pyr, out = K.reference_pyramid(h, w, nlevels, scale, simd), set()
    for l in range(1, nlevels):
        if K.level_kind(h, w, nlevels, scale, l) != "area":
            continue
        (sw, sh), (dw, dh) = K.level_sizes(h, w, nlevels, scale)[l - 1:l + 1]
        s = pyr[l - 1].astype(np.int64)
        sums = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2])[:, K.xvec(sw, sh, dw, dh, simd):]
        out |= {int(q) & 1 for q in (sums[sums % 4 == 2] // 4).ravel()}
    return out


def reached(case) -> set:
    """The names of everything a case reaches."""
    h, w, nlevels, scale, simd, strips = case
    geo = (h, w, nlevels, scale)
    sizes, out = K.level_sizes(*geo), set()
    htop = sizes[-1][1]
    n = _strips(case)
    first = K.cascade_strips(htop, nlevels, K.NOMINAL_CUS, 1)
    ngrp = [K.groups(s[0]) for s in sizes[1:]]
    if strips == K.AUTO:
        if n and n > first and max(ngrp) <= K.CAS_GROUPS:
            out.add("search: a later count fits")
        if not n and first <= htop and max(ngrp) <= K.CAS_GROUPS:
            out.add("search: no count fits")
        if htop < 4 and not n and first > htop:
            out.add("search: fewer top rows than the smallest count")
        if max(ngrp) == K.CAS_GROUPS and n:
            out.add("width: the most groups a cascade takes")
        if max(ngrp) == K.CAS_GROUPS + 1 and not n:
            out.add("width: one group too many")
            if K.level_kind(*geo, 1) == "area":
                out.add("width: one group too many, area")
        if n and w == 12000:
            out.add("width: the longest source rows")
    if not n:
        return out
    cs = K.resize_strips(*geo, n)
    runs = [K.staged_run(*geo, n, k) for k in range(n)]
    out |= {f"src_sh {r['src_sh']}" for r in runs}
    for r in runs:
        out |= {"run: one pass, filled"} if r["ndw"] == K.PASS_DWORDS else set()
        out |= {"run: one dword over a pass"} if r["ndw"] == K.PASS_DWORDS + 1 else set()
        out |= {"run: three passes"} if r["passes"] >= 3 else set()
        out |= {"run: threads that stage nothing"} if r["ndw"] < K.CAS_THREADS else set()
    out |= {"strips: one"} if n == 1 else set()
    out |= {"strips: one top row each"} if n == htop and n > 1 else set()
    if n >= 3:
        out.add("strips: first and last")
        if any(all(cs["chi"][l][k] > cs["own"][l][k + 1] for l in range(1, nlevels - 1)) for k in range(1, n - 1)) \
                and nlevels >= 3:
            out.add("strips: a middle strip with a halo at every level below the top")
    for l in range(1, nlevels):
        for k in range(n):
            rows = cs["chi"][l][k] - cs["clo"][l][k]
            out.add("rows: fewer than waves" if rows < K.CAS_WAVES else "rows: one per wave" if rows == K.CAS_WAVES else
                    "rows: one more than waves" if rows == K.CAS_WAVES + 1 else "rows: several rounds")
        wl = sizes[l][0]
        out |= {"groups: 64"} if ngrp[l - 1] == 64 and wl == 256 else set()
        out |= {"groups: 65"} if ngrp[l - 1] == 65 else set()
        out |= {"groups: at most 4"} if ngrp[l - 1] <= 4 else set()
        out |= {f"width {wl % 4} mod 4"} if wl % 4 else set()
        kind = K.level_kind(*geo, l)
        out.add(f"step: {kind}")
        tails = K.tail_groups(*geo, simd, l)
        if len(tails) == ngrp[l - 1] and simd == 0:
            out.add("tail: every group")
        elif 0 < len(tails) < ngrp[l - 1]:
            out.add("tail: the last groups")
        (sw, sh), (dw, dh) = sizes[l - 1:l + 1]
        if simd and kind != "area" and K.xvec(sw, sh, dw, dh, simd) % simd == simd // 2:
            out.add("tail: after a half step")
    if "step: area" in out and _area_ties(case) == {0, 1}:
        out.add("step: area sums that round half to even, both ways")
    if "step: wide" in out and scale == 3.0:
        out.add("step: wide at 3.0")
    out.add(f"levels: {nlevels if nlevels <= 4 else 'deep'}")
    out.add(f"simd {simd}")
    return out


CASES_FOR = {
    "src_sh 0": K.STRIPS[:2], "src_sh 1": K.STRIPS[:2], "src_sh 2": K.STRIPS[:2], "src_sh 3": K.STRIPS[:2],
    "run: one pass, filled": K.STAGING[1:2],
    "run: one dword over a pass": K.STAGING[2:3],
    "run: three passes": K.STAGING[3:4],
    "run: threads that stage nothing": K.STAGING[:1],
    "strips: one": K.STAGING[1:],
    "strips: one top row each": K.STRIPS[:1],
    "strips: a middle strip with a halo at every level below the top": K.STRIPS[2:],
    "strips: first and last": K.STRIPS,
    "rows: fewer than waves": K.STRIPS[:2],
    "rows: one per wave": K.STRIPS[1:2],
    "rows: one more than waves": K.STRIPS[1:2],
    "rows: several rounds": K.STRIPS[2:],
    "groups: 64": K.GROUPS[:1],
    "groups: 65": K.GROUPS[1:3],
    "groups: at most 4": K.GROUPS[3:],
    "width 1 mod 4": K.STAGING[:1] + K.GROUPS[:1],
    "width 2 mod 4": K.GROUPS[1:3],
    "width 3 mod 4": K.STAGING[:1] + K.GROUPS[1:3],
    "step: area": K.STEPS[:3],
    "step: area sums that round half to even, both ways": K.STEPS[:1],
    "step: wide": K.STEPS[3:6],
    "step: wide at 3.0": K.STEPS[4:6],
    "step: linear": K.STEPS[6:],
    "tail: every group": [K.STEPS[0], K.STEPS[5], K.STEPS[7]],
    "tail: the last groups": [K.STEPS[1], K.STEPS[2], K.STEPS[3], K.STEPS[8]],
    "tail: after a half step": [K.STEPS[6], K.STEPS[8]],
    "simd 0": [K.STEPS[0], K.STEPS[5], K.STEPS[7]],
    "simd 16": K.STAGING,
    "simd 32": [K.STEPS[2], K.STEPS[6], K.STEPS[8]],
    "levels: 2": K.STAGING[1:],
    "levels: 3": K.STRIPS[:2],
    "levels: 4": K.STRIPS[2:],
    "levels: deep": K.STEPS[9:],
    "width: the most groups a cascade takes": K.WIDTH[:1],
    "width: one group too many": K.WIDTH[1:3],
    "width: one group too many, area": K.WIDTH[2:3],
    "width: the longest source rows": K.WIDTH[3:],
    "search: a later count fits": K.SEARCH[:1],
    "search: no count fits": K.SEARCH[1:2],
    "search: fewer top rows than the smallest count": K.SEARCH[2:],
}


@pytest.mark.parametrize("target", sorted(CASES_FOR))
def test_every_target_is_reached_by_its_cases(target):
    cases = CASES_FOR[target]
    assert cases, target
    for case in cases:
        assert case in K.ALL and target in reached(case), (target, K.case_id(case), sorted(reached(case)))


def test_every_case_serves_a_target():
    listed = {c for cases in CASES_FOR.values() for c in cases}
    assert set(K.ALL) - set(K.ORDINARY) <= listed
    for case in K.ORDINARY:  # the path test's ordinary geometries take the cascade at its first count
        h, w, nlevels, scale, simd, strips = case
        htop = K.level_sizes(h, w, nlevels, scale)[-1][1]
        for n in (1, 2):
            assert K.chosen_strips(h, w, nlevels, scale, K.NOMINAL_CUS, n) == K.cascade_strips(htop, nlevels, K.NOMINAL_CUS, n)


def test_the_issues_figures():
    """The figures the cases were proposed with: the strip counts and LDS totals of the search and width cases."""
    assert K.chosen_strips(300, 4800, 5, 1.2, 256, 1) == 116 and K.cascade_strips(145, 5, 256, 1) == 48
    assert K.chosen_strips(300, 4800, 6, 1.2, 256, 1) == 0
    assert K.chosen_strips(120, 4915, 3, 1.2, 256, 1) == 27
    assert K.resize_strips(120, 4915, 3, 1.2, 27)["lds"] == 128656
    assert K.chosen_strips(120, 4917, 3, 1.2, 256, 1) == 0          # 1 025 groups
    assert K.chosen_strips(600, 4500, 8, 1.2, 256, 1) == 0          # tests/test_gpu_extract.py's wide image: the LDS
    assert K.chosen_strips(4500, 2500, 8, 1.2, 256, 1) == 420       # its tall image: past the first count of 256
    assert K.staged_run(128, 256, 2, 1.2, 1, 0)["ndw"] == 8192 == K.PASS_DWORDS
    assert K.staged_run(230, 300, 2, 1.2, 1, 0)["passes"] == 3


def _strip_counts(case) -> set:
    h, w, nlevels, scale, simd, strips = case
    counts = {_strips(case)} | {K.chosen_strips(h, w, nlevels, scale, cus, n) for cus in (K.NOMINAL_CUS, 304) for n in (1, 2)}
    return counts - {0}


@pytest.mark.parametrize("case", K.ALL + [K.BATCH + (1.2, 16, s) for s in K.BATCH_STRIPS], ids=K.case_id)
def test_strip_tables(case):
    """Owned ranges partition every level; a strip's computed range holds its owned rows and both source rows of
    every row it computes at the next level, and never begins before its owned rows; the staged run holds the
    source rows of its level-1 rows; every buffer holds its rows; every table entry fits int16."""
    h, w, nlevels, scale, simd, _ = case
    sizes, yt = K.level_sizes(h, w, nlevels, scale), K._ytabs(h, w, nlevels, scale)
    for l in range(1, nlevels):  # steps above 1: no sy0 / sy1 is clipped at the border
        (sw, sh), (dw, dh) = sizes[l - 1:l + 1]
        assert yt[l][0][0] >= 0 and yt[l][1][-1] <= sh - 1 and all(b == a + 1 for a, b in zip(*yt[l]))
    for n in _strip_counts(case):
        cs = K.resize_strips(h, w, nlevels, scale, n)
        assert cs and cs["lds"] <= K.LDS_LIMIT and cs["off_b"] % 16 == 0 and cs["off_x"] % 16 == 0
        own, clo, chi = cs["own"], cs["clo"], cs["chi"]
        for l in range(1, nlevels):
            hl, size = sizes[l][1], (cs["off_b"] if l % 2 == 0 else cs["off_x"] - cs["off_b"])
            assert own[l][0] == 0 and own[l][n] == hl and all(a <= b for a, b in zip(own[l], own[l][1:]))
            for k in range(n):
                assert 0 <= clo[l][k] == own[l][k] <= own[l][k + 1] <= chi[l][k] <= hl < 2 ** 15
                assert clo[l][k] < chi[l][k]
                assert (chi[l][k] - clo[l][k]) * K.pitch(sizes[l][0]) + 12 <= size  # + the taps' over-read
                if l + 1 < nlevels:
                    for r in range(clo[l + 1][k], chi[l + 1][k]):
                        assert clo[l][k] <= yt[l + 1][0][r] <= yt[l + 1][1][r] < chi[l][k], (n, l, k, r)
        for k in range(n):
            for img in range(4):
                run = K.staged_run(h, w, nlevels, scale, n, k, img)
                assert 4 * run["ndw"] + 12 <= cs["off_b"]
                for r in range(clo[1][k], chi[1][k]):
                    assert run["ys_lo"] <= yt[1][0][r] <= yt[1][1][r] <= run["ys_hi"] < h


def test_every_case_is_accepted_by_the_oracle():
    for case in K.ALL:
        h, w, nlevels, scale, simd, _ = case
        pyr = K.reference_pyramid(h, w, nlevels, scale, simd)
        assert len(pyr) == nlevels and pyr[0].shape == (h, w)
        assert [p.shape[::-1] for p in pyr] == list(K.level_sizes(h, w, nlevels, scale))


def test_forced_counts_fit():
    for case in K.ALL:
        h, w, nlevels, scale, simd, strips = case
        if strips != K.AUTO:
            assert K.forced_strips(h, w, nlevels, scale, strips) == strips, K.case_id(case)


def test_batch_geometry_and_contents():
    h, w, nlevels = K.BATCH
    assert (w * h) % 4 in (1, 3) and nlevels == S.MIXED_NLEVELS
    top = K.level_sizes(h, w, nlevels, 1.2)[-1][1]
    assert top in K.BATCH_STRIPS and len(set(K.BATCH_STRIPS)) >= 2
    # every misalignment of the staged run in a later image of the batch, at each forced count
    for n in K.BATCH_STRIPS:
        assert K.forced_strips(h, w, nlevels, 1.2, n) == n
        if n > 1:
            for img in range(1, 6):
                assert len({K.staged_run(h, w, nlevels, 1.2, n, k, img)["src_sh"] for k in range(n)}) >= 3
        assert {K.staged_run(h, w, nlevels, 1.2, n, 0, img)["src_sh"] for img in range(6)} == {0, 1, 2, 3}
    for pairs in (1, 3):
        first, second = S.mixed_batch(h, w, pairs, *K.BATCH_FIRST), S.mixed_batch(h, w, pairs, *K.BATCH_SECOND)
        for a, b, ra, rb in zip(first.images, second.images, first.image_refs, second.image_refs):
            assert (a != b).any()
            # results that depend on the resized levels
            assert ra.levels_with_keypoints() - {0} and rb.levels_with_keypoints() - {0}
        assert all((r.status == 1).any() for r in first.pair_refs + second.pair_refs)
