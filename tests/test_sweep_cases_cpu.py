"""The inputs of tests/test_gpu_sweep.py meet the conditions their cases are built for (oracle and restatement
only, no GPU): without them a GPU comparison could pass on inputs that never reach the code it is meant for."""
import numpy as np
import pytest

import sweep_cases as S


def _levels(img, nlevels):
    return S.ImageRef(img, nlevels).levels_with_keypoints()


@pytest.mark.parametrize("name", sorted(S.LISTS))
def test_every_geometry_is_accepted_by_the_oracle(name):
    """OracleExtractor raises ValueError where the reference's DistributeOctTree refuses a geometry."""
    for h, w, nlevels in S.LISTS[name]:
        for c in S.CONTENT_ORDER:
            S.ImageRef(S.content(c, 1, h, w), nlevels)


def test_geometry_lists_cover_the_residues():
    assert len(S.WIDTHS) == 72 and len(S.HEIGHTS) == 72
    ws = sorted({w for _, w, _ in S.WIDTHS})
    assert ws == list(range(96, 132)) and {w % 30 for w in ws} == set(range(30)) and {w % 4 for w in ws} == {0, 1, 2, 3}
    assert {(h * w) % 4 for h, w, _ in S.WIDTHS} == {0, 1, 2, 3}
    assert sorted({h for h, _, _ in S.HEIGHTS}) == list(range(62, 98))
    assert [(h * w) % 4 for h, w in S.MIXED_GEOMETRIES] == [0, 2, 1]


def test_widths_noise_has_keypoints_on_every_level():
    for h, w, nlevels in S.WIDTHS:
        assert _levels(S.noise(3, h, w), nlevels) == {0, 1, 2}, (h, w)


def test_resize_tails_reach_their_residues_and_level_1():
    from oracle.oracle import OracleExtractor
    for (h, w, nlevels), res in zip(S.RESIZE_TAILS, S.RESIZE_TAIL_RESIDUES):
        w1, h1 = OracleExtractor(**S.params(nlevels)).level_sizes(w, h)[1]
        assert ((w1 + 3) // 4) % 64 == res and (w1 + 3) // 4 >= 64, (w, w1)
        for c in ("noise", "natural"):
            assert {0, 1} <= _levels(S.content(c, 2, h, w), nlevels), (w, c)


def test_heights_span_one_level_to_three():
    per_geo = [len(_levels(S.noise(4, h, w), nlevels)) for h, w, nlevels in S.HEIGHTS]
    assert min(per_geo) == 1 and max(per_geo) >= 3, per_geo
    # the lowest height is the lowest at all: one row fewer and the oracle finds nothing
    assert len(S.ImageRef(S.noise(4, 61, 130), 4).kps) == 0


def test_sweep_right_views_are_matched():
    """shifted(left, 3) gives the restatement something to match at both ends of the width list."""
    for h, w, nlevels in (S.WIDTHS[0], S.WIDTHS[-1], S.RESIZE_TAILS[0]):
        for c in ("noise", "natural", "coarse"):
            left = S.content(c, 5, h, w)
            ref = S.PairRef(S.ImageRef(left, nlevels), S.ImageRef(S.shifted(left, 3), nlevels))
            assert (ref.status == 1).any(), (h, w, c)


@pytest.mark.parametrize("hw", S.MIXED_GEOMETRIES)
def test_mixed_batch_conditions(hw):
    h, w = hw
    mb = S.mixed_batch(h, w, 8)
    assert sorted(mb.kinds) == sorted(S.PAIR_KINDS)
    zero_disparity = 0
    for p, kind in enumerate(mb.kinds):
        left, right, pr = mb.image_refs[2 * p], mb.image_refs[2 * p + 1], mb.pair_refs[p]
        if kind in S.BOTH_SIDES:
            assert len(left.kps) > 0 and len(right.kps) > 0, kind
            assert (pr.status == 1).any(), kind
            zero_disparity += int((pr.status == 2).sum())
        else:
            assert len(left.kps) == 0 or len(right.kps) == 0, kind
            assert (len(left.kps) == 0) == kind.startswith("flat"), kind
            assert (len(right.kps) == 0) == kind.endswith("flat"), kind
            assert len(pr.status) == len(left.kps) and not pr.status.any() and (pr.match_r == -1).all(), kind
            assert (pr.u_right == -1).all() and (pr.depth == -1).all(), kind
    assert zero_disparity > 0  # identical pairs (lattice, binary): the Python-double substitution


def test_long_mixed_batch_moves_the_kinds_over_the_offsets():
    """Over 32 pairs every kind stands at an even and at an odd pair index (image byte offsets 2 p W H)."""
    seen = {(S.pair_kind(p), p % 2) for p in range(32)}
    assert seen == {(k, r) for k in S.PAIR_KINDS for r in (0, 1)}
    assert all(sorted(S.pair_kind(p) for p in range(8 * c, 8 * c + 8)) == sorted(S.PAIR_KINDS) for c in range(6))
