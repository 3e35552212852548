"""The inputs of tests/test_gpu_bow_assemble.py contain what they are for (no GPU): every fact below is computed
with VocabOracle alone."""
import numpy as np
import pytest

import bow_assemble_cases as AC
import vocab_synth as VS


def descents(o, frame):
    return [o.descend(q, o.L - AC.LEVELS_UP) for q in frame]


def test_geometry_matches_the_sources():
    c = AC.source_constants()
    assert c["ORBFE_BOW_MAX_FRAME"] == AC.MAX_FRAME >= 8192
    assert c["kBowSmall"] == AC.SMALL_FRAME and c["kBowItems"] == AC.ITEMS
    assert AC.WORKGROUPS == (AC.SMALL_FRAME // AC.ITEMS, AC.MAX_FRAME // AC.ITEMS)
    from pyorbslam_amd import _lib
    assert _lib.ORBFE_BOW_MAX_FRAME == AC.MAX_FRAME


def test_every_frame_length_edge_is_present():
    want = set(AC.ISSUE_LENGTHS) | {AC.MAX_FRAME}
    for p in AC.WORKGROUPS + (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        want |= {p - 1, p, p + 1}
    want |= {AC.MAX_FRAME - 1}
    assert want <= set(AC.EDGE_LENGTHS) and max(AC.EDGE_LENGTHS) == AC.MAX_FRAME
    for tree, seed, pool in ((AC.small_tree(), 41, 600), (AC.wide_tree(), 43, 6000)):
        frames = AC.length_frames(tree, seed, pool)
        lens = [len(f) for f in frames]
        assert sorted(set(lens)) == AC.EDGE_LENGTHS
        assert lens[0] == 0 and lens[-1] == 0 and 0 in lens[1:-1]     # empty first, last and between
        assert all(f.dtype == np.uint8 and f.shape[1:] == (32,) for f in frames)


def test_small_tree_is_mostly_duplicates_and_wide_tree_keeps_everything():
    small, wide = AC.small_tree(), AC.wide_tree()
    assert 4 <= int(small["is_leaf"].sum()) <= 64 and (small["weight"][small["is_leaf"] > 0] == 0).any()
    o = AC.PoolOracle(small)
    f = AC.length_frames(small, 41, 600)
    big = max(f, key=len)
    bv, fv = o.transform(big, AC.LEVELS_UP)
    assert len(bv) <= 64 and sum(len(v) for v in fv.values()) < len(big)     # duplicates and dropped features
    assert any(n < 0 for _, n, _ in descents(o, big[:500]))                 # descents above the node level
    # wide: all weights positive, so every frame's kept features are all of it: the sort sees the frame lengths
    assert bool(np.all(wide["weight"][wide["is_leaf"] > 0] > 0)) and int(wide["is_leaf"].sum()) == 8000
    ow = AC.PoolOracle(wide)
    fw = AC.length_frames(wide, 43, 6000)
    for frame in (fw[1], fw[len(fw) // 2 + 2]):
        bv, fv = ow.transform(frame, AC.LEVELS_UP)
        assert sum(len(v) for v in fv.values()) == len(frame)
        assert len(bv) > len(frame) // 4                                     # few duplicates


def test_special_frames_contain_what_they_are_named_for():
    t = AC.small_tree()
    o = AC.PoolOracle(t)
    fr = AC.special_frames(t, o, 51)
    names = list(fr)
    d = {k: descents(o, v) for k, v in fr.items()}
    # a frame that starts above the node level directly after one that ends with a valid node
    assert names.index("starts_short") == names.index("ends_valid") + 1
    end_node = d["ends_valid"][-1][1]
    assert end_node > 0 and d["ends_valid"][-1][2] > 0
    assert d["starts_short"][0][1] < 0 and d["starts_short"][1][1] < 0 and d["starts_short"][0][2] > 0
    fv = o.transform(fr["starts_short"], AC.LEVELS_UP)[1]
    assert fv[0][:2] == [0, 1] and 0 not in fv.get(end_node, [])     # node 0, not the previous frame's node
    # a run of >= 65 features of one word, and a frame that is one word throughout
    words = [w for w, _, wt in d["long_run"] if wt > 0]
    assert max(words.count(w) for w in set(words)) >= 65 and len(set(words)) > 1
    assert len({w for w, _, _ in d["one_word"]}) == 1 and len(fr["one_word"]) == 300
    assert all(wt > 0 for _, _, wt in d["one_word"]) and len(o.transform(fr["one_word"], AC.LEVELS_UP)[0]) == 1
    # dropped features between kept ones
    keep = [wt > 0 for _, _, wt in d["holes"]]
    assert keep[0] and not keep[1] and keep[2] and any(keep[i] and not keep[i + 1] and keep[i + 2]
                                                       for i in range(len(keep) - 2))
    # only dropped features
    assert len(fr["all_dropped"]) == 77 and not any(wt > 0 for _, _, wt in d["all_dropped"])
    assert o.transform(fr["all_dropped"], AC.LEVELS_UP) == ({}, {})


def test_patched_tree_reaches_its_negative_and_nan_leaves():
    t, neg, nan = AC.patched_tree()
    assert t["weight"][neg] < 0 and np.isnan(t["weight"][nan])
    o = AC.PoolOracle(t)
    pool = VS.query_descriptors(t, 33, 400)
    w = np.array([o.descend(q, o.L - AC.LEVELS_UP)[2] for q in pool])
    assert (w < 0).any() and np.isnan(w).any() and (w > 0).any()
    bv, fv = o.transform(pool, AC.LEVELS_UP)
    kept = sorted(i for v in fv.values() for i in v)
    assert kept == np.flatnonzero(w > 0).tolist()            # negative and NaN weights drop the feature
    assert all(x > 0 for x in bv.values())
