"""CPU pre-conditions of tests/test_gpu_bow.py: the inputs of tests/bow_cases.py reach the loop iterations they
aim at, and the oracles are pinned on them (VocabOracle against the reference's own outputs on the wide tree,
tests/golden/vocab_wide.npz; the host side of the native library where no launch is involved)."""
import numpy as np
import pytest

import bow_cases as BC
import kfdb_oracle as KO
import vocab_synth as VS
from oracle.vocab_oracle import VocabOracle
from test_vocab import golden_outputs, same


@pytest.fixture(scope="module")
def wide():
    z, tree, q = BC.wide_golden()
    return z, tree, q, z["query_node"].astype(np.int64), BC.trace(tree, q)


def test_wide_tree_is_what_the_golden_recorded(wide):
    z, tree, q, ids, _ = wide
    t = BC.wide_tree(BC.WIDE_SEED)
    for key in ("parent", "is_leaf", "desc", "weight"):
        assert np.array_equal(t[key], z[key]), key
    assert (int(z["k"]), int(z["L"])) == (10, 2) and z["levels_up"].tolist() == [0, 1, 2]
    lq, lids = BC.leaf_queries(t, 14)
    assert np.array_equal(q, lq) and np.array_equal(ids, lids) and sorted(ids.tolist()) == list(range(66, 4730))
    fan = np.bincount(tree["parent"][1:], minlength=len(tree["parent"]))
    assert fan[0] == 65 == BC.WIDE_ROOT
    assert fan[1:66].tolist() == [BC.FANOUT[i % 12] for i in range(65)]
    assert set(BC.FANOUT) == set(fan[1:66].tolist()) and fan[66:].max() == 0
    assert len(tree["parent"]) == 4730 and len(q) == 4664
    assert (BC.ROOT / "tests" / "golden" / "vocab_wide.npz").stat().st_size < 330_000   # no larger than the others


def test_oracle_matches_reference_on_wide_tree(wide):
    z, tree, q, _, _ = wide
    o = VocabOracle(z["parent"], z["is_leaf"], z["desc"], z["weight"], 2)
    for lu in (0, 1, 2):
        same(o.transform(q, lu), *golden_outputs(z, lu))


def test_wide_queries_reach_the_pass_loop(wide):
    """Every query ends under its own parent, on the first child equal to it; at least 100 queries each win at
    position >= 32, tie across passes and tie with a lower lane; every fan-out above 33 supplies all three."""
    z, tree, q, ids, tr = wide
    o = VocabOracle(z["parent"], z["is_leaf"], z["desc"], z["weight"], 2)
    fan = np.bincount(tree["parent"][1:], minlength=len(tree["parent"]))
    first_child = np.concatenate([[1], 1 + np.cumsum(fan)[:-1]])   # breadth-first numbering
    count = {"late": 0, "cross": 0, "lower": 0}
    per_fan = {f: [0, 0, 0] for f in BC.FANOUT if f > 32}
    for (levels, node), x, i in zip(tr, q, ids.tolist()):
        assert len(levels) == 2 and levels[1][0] == tree["parent"][i]           # the intended parent
        assert np.array_equal(tree["desc"][node], x) and node <= i                # the first equal child
        assert o.descend(x, 1) == (int(o.word[node]), int(tree["parent"][i]), float(tree["weight"][node]))
        assert node == first_child[levels[1][0]] + levels[1][1]
        late, cross, lower = BC.categories(levels[1:])   # at the leaf level alone
        count["late"] += late
        count["cross"] += cross
        count["lower"] += lower
        f = int(fan[levels[1][0]])
        if f > 32:
            for k, hit in enumerate((late, cross, lower)):
                per_fan[f][k] += hit
    print(count, per_fan)
    assert all(v >= 100 for v in count.values()), count
    # fan-out 33 has a single child in its second pass (position 32, which the planting rule leaves unique): it
    # can win there but has nothing to tie with; every wider node supplies all three
    assert per_fan.pop(33)[0] > 0
    assert sorted(per_fan) == [63, 64, 65, 96, 97, 129, 300] and all(min(v) > 0 for v in per_fan.values()), per_fan
    # the root's 65 children span three passes too
    assert sum(levels[0][1] >= 32 for levels, _ in tr) >= 100


def test_wide_tree_text_roundtrip(wide, tmp_path):
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    z, tree, _, _, _ = wide
    path = tmp_path / "wide.txt"
    VS.write_text(tree, path)
    v = TemplatedVocabulary()
    assert v.load_from_text_file(path) is True
    info = v.info()
    assert (info.k, info.L, info.max_children, info.n_nodes, info.depth) == (10, 2, 300, 4730, 2)
    a = v.node_arrays()
    assert np.array_equal(a["parent"], tree["parent"]) and np.array_equal(a["is_leaf"], tree["is_leaf"])
    assert np.array_equal(a["desc"][1:], tree["desc"][1:]) and np.array_equal(a["weight"], tree["weight"])
    assert v.size() == int(z["size"]) == 4664


def test_flat_tree_and_the_fan_out_limit():
    from pyorbslam_amd._lib import ORBFE_EINVAL, OrbfeError
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    t = BC.flat_tree(61)
    v = TemplatedVocabulary(k=10, L=1).from_arrays(t["parent"], t["is_leaf"], t["desc"], t["weight"])
    info = v.info()
    assert (info.max_children, info.n_words, info.depth) == (65535, 65535, 1)
    # the planted pairs straddle 2^15 and end at the last position; a copy of either member wins at the first
    q, pos = BC.flat_queries(t, 62)
    assert len(q) == 96 and any(a < 32768 <= b for a, b in t["pairs"]) and (3, 65534) in t["pairs"]
    first_of = {b: a for a, b in t["pairs"]}
    o = VocabOracle(t["parent"], t["is_leaf"], t["desc"], t["weight"], 1)
    won = [o.descend(x, 1)[0] for x in q]
    assert won == [first_of.get(p, p) for p in pos.tolist()]       # word id == child position here
    assert sum(w >= 32768 for w in won) >= 32 and 65534 in pos.tolist() and 3 in won
    # one child more is refused by the host, before anything is laid out for the device
    n = 65536
    with pytest.raises(OrbfeError) as e:
        TemplatedVocabulary(k=10, L=1).from_arrays(np.zeros(n + 1, np.int32), np.ones(n + 1, np.uint8),
                                                   np.zeros((n + 1, 32), np.uint8), np.ones(n + 1))
    assert e.value.code == ORBFE_EINVAL and "65535" in str(e.value)


def test_mismatched_flags_reach_word_zero():
    t = BC.mismatched_tree(71)
    n = len(t["parent"])
    has_child = np.zeros(n, bool)
    has_child[t["parent"][1:]] = True
    flagged_inner = np.flatnonzero(has_child & (t["is_leaf"] > 0))
    loose = np.flatnonzero(~has_child & (t["is_leaf"] == 0) & (t["weight"] > 0))
    loose = loose[loose > 0]
    assert len(flagged_inner) >= 0.05 * n and len(loose) >= 0.05 * n, (n, len(flagged_inner), len(loose))
    q = VS.query_descriptors(t, 72, 600)
    ends = [node for _, node in BC.trace(t, q)]
    on_loose = [e for e in ends if e in set(loose.tolist())]
    assert len(on_loose) >= 20 and len(set(on_loose)) > 1      # word 0 collects weight from several nodes
    o = VocabOracle(t["parent"], t["is_leaf"], t["desc"], t["weight"], t["L"])
    assert all(o.descend(x, 2)[0] == 0 for x, e in zip(q, ends) if e in set(loose.tolist()))
    bv, _ = o.transform(q, 2)
    w0 = [float(t["weight"][e]) for e in ends if o.word[e] == 0 and t["weight"][e] > 0]
    total = sum(float(t["weight"][e]) for e in ends)
    assert len(set(on_loose)) > 1 and abs(bv[0] - sum(w0) / total) < 1e-12
    # the flagged inner nodes shift the word ids of everything after them
    assert not np.array_equal(o.word, VocabOracle(t["parent"], BC.ragged_tree()["is_leaf"], t["desc"], t["weight"],
                                                  t["L"]).word)


def test_long_database_gives_waves_a_second_slot():
    k = BC.kernel_constants()
    waves = k["kBowWaves"] * k["kBowMaxBlocks"]
    assert BC.LONG_SLOTS > waves and BC.LONG_SLOTS - waves == 13       # some waves take two slots, others one
    assert k["kBowLdsWords"] == 8192 and 64 * k["kBowUnroll"] == 256   # what the length lists straddle
    q, vecs, erased = BC.long_database()
    assert len(vecs) == BC.LONG_SLOTS and len(q) == BC.LONG_NQ
    assert [len(v) for v in vecs[:8192]] == [s % 71 for s in range(8192)]
    assert 100 < len(erased) < 250 and not set(erased) & set(BC.LONG_KEEP)
    live = [None if s in set(erased) else v for s, v in enumerate(vecs)]
    common, first, score = KO.query_arrays(live, q)
    assert common[8192] == 200 and all(common[s] > 0 for s in BC.LONG_KEEP)
    # a stale accumulator shows only where the wave's first slot left something behind and the second differs
    lo, hi = np.arange(1, 13), np.arange(8193, 8205)
    both = [(a, b) for a, b in zip(lo, hi) if common[a] > 0 and live[b] is not None]
    assert len(both) >= 8 and any(first[a] != first[b] for a, b in both)


def test_score_inputs_reach_the_pass_and_chunk_boundaries():
    for nq in (300, 5000):
        q, vecs = BC.pass_world(nq, seed=nq)
        assert [len(v) for v in vecs] == BC.PASS_LENGTHS * 2 and len(q) == nq
        common, first, _ = KO.query_arrays(vecs, q)
        # hits in the first and in the last 256-word pass of every length, the one-word last pass of 257 and
        # 513 included (the second half of the world shares every word it can)
        last_pass = {}
        for v, c in zip(vecs, common):
            hit = np.flatnonzero([w in q for w in v])
            assert c == len(hit) > 0 and hit[0] < 64
            last_pass[len(v)] = last_pass.get(len(v), False) or hit[-1] >= (len(v) - 1) // 256 * 256
        assert all(last_pass.values()), last_pass
    q, vecs = BC.single_shared_world()
    common, first, _ = KO.query_arrays(vecs, q)
    assert len(q) == 300 and common.tolist() == [1] * 8
    for v, p, f in zip(vecs, BC.SINGLE_POSITIONS, first.tolist()):
        assert len(v) == 600 and list(v)[p] == f == 1000 * p and list(v) == sorted(v)
    for nq in BC.EDGE_QUERY_LENGTHS:
        q, vecs = BC.extended_world(nq, seed=nq)
        assert len(q) == nq and {len(v) for v in vecs} >= set(BC.PASS_LENGTHS)


def test_odd_weights_keep_their_bits_in_the_oracle():
    q, vecs = BC.odd_weight_world()
    seen = set(q.values())
    for v in vecs:
        seen |= set(v.values())
    assert seen == set(BC.ODD_WEIGHTS) and 5e-324 in seen and -1e300 in seen
    assert all(np.isfinite(x) for x in seen)
    common, _, score = KO.query_arrays(vecs, q)
    assert np.all(common > 0) and np.all(np.isfinite(score))
    # the scores are not all zeros or huge: subnormal results survive in Python double arithmetic
    tiny = np.abs(score[(score != 0) & (np.abs(score) < 2.3e-308)])
    assert len(tiny) > 0 and np.sum(np.abs(score) > 1e299) > 0 and len(np.unique(score)) > 10
