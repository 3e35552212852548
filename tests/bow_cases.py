"""Inputs of the bag-of-words boundary tests (tests/test_gpu_bow.py) and of their CPU pre-conditions
(tests/test_bow_cases_cpu.py): vocabulary trees whose nodes are wider than one 32-lane pass of
k_vocab_descend, and BoW vectors that make k_bow_score take a second slot per wave, a second 256-word pass
and the last LDS-resident query lengths.  Pure numpy, deterministic by seed.

The builders aim at loops that run once under every other tree and database of the suite; the CPU test file
shows that they reach them (which child wins, which ties exist, which waves take two slots)."""
from __future__ import annotations

import re
from collections import OrderedDict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
N_WORDS = 1_000_003   # the large vocabulary of tests/test_kfdb_gpu.py

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


# ---- vocabulary trees -------------------------------------------------------------------------------------------
FANOUT = [1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 129, 300]
WIDE_ROOT = 65
WIDE_SEED = 21


def flip_bits(rng, base: np.ndarray, n: int, bits: int) -> np.ndarray:
    """n copies of the 32-byte descriptor base, each with `bits` distinct random bits flipped."""
    out = np.repeat(base[None, :], n, axis=0).copy()
    for r in range(n):
        for b in rng.choice(256, bits, replace=False).tolist():
            out[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def plant_duplicates(d: np.ndarray) -> np.ndarray:
    """Equal children of one node, by child position p (ascending, so copies of copies stay equal):
      p >= 32 and p % 3 == 0           child p = child p - 32   same lane of the 32-lane group, one pass later
      else p >= 20 and p % 5 == 0      child p = child p - 13   a lower lane in a later pass whenever
                                                                 [p - 13, p] holds a multiple of 32
    The first of two equal children must win (TemplatedVocabulary.py:143-150 takes a strict minimum)."""
    for p in range(len(d)):
        if p >= 32 and p % 3 == 0:
            d[p] = d[p - 32]
        elif p >= 20 and p % 5 == 0:
            d[p] = d[p - 13]
    return d


def wide_tree(seed: int = WIDE_SEED, n_level1: int = WIDE_ROOT) -> dict:
    """Depth 2, n_level1 children under the root, FANOUT[i % 12] leaves under level-1 node i, numbered
    breadth-first.  Children are their parent with 20 bits flipped (any two siblings differ in about 40, a leaf
    and another level-1 node in about 60), so a copy of a leaf descends to that leaf's parent and, there, to the
    first child equal to it.  The header k = 10 is what the file claims, not what the nodes have: like the
    reference, the loader checks the header alone."""
    rng = np.random.Generator(np.random.PCG64(seed))
    root = rng.integers(0, 256, 32, dtype=np.uint8)
    level1 = flip_bits(rng, root, n_level1, 20)
    parent, desc = [np.zeros(1 + n_level1, np.int32)], [np.zeros((1, 32), np.uint8), level1]
    for i in range(n_level1):
        n = FANOUT[i % len(FANOUT)]
        desc.append(plant_duplicates(flip_bits(rng, level1[i], n, 20)))
        parent.append(np.full(n, 1 + i, np.int32))
    parent = np.concatenate(parent)
    n_nodes = len(parent)
    is_leaf = np.zeros(n_nodes, np.uint8)
    is_leaf[1 + n_level1:] = 1
    weight = np.zeros(n_nodes, np.float64)
    w = rng.uniform(0.05, 6.0, n_nodes - 1 - n_level1)
    w[rng.random(len(w)) < 0.03] = 0.0
    weight[1 + n_level1:] = w
    return dict(k=10, L=2, parent=parent, is_leaf=is_leaf, desc=np.concatenate(desc), weight=weight)


def leaf_queries(tree: dict, seed: int):
    """Every childless node's descriptor once, in a seeded order: (queries [n, 32], their node ids)."""
    parent = np.asarray(tree["parent"])
    has_child = np.zeros(len(parent), bool)
    has_child[parent[1:]] = True
    ids = np.flatnonzero(~has_child)
    ids = ids[ids > 0]
    ids = ids[np.random.Generator(np.random.PCG64(seed)).permutation(len(ids))]
    return np.ascontiguousarray(tree["desc"][ids]), ids


def wide_golden():
    """tests/golden/vocab_wide.npz: (the npz, its tree, its queries).  The fixture keeps the queries as the ids of
    the nodes whose descriptors they are."""
    z = np.load(ROOT / "tests" / "golden" / "vocab_wide.npz", allow_pickle=False)
    tree = dict(k=int(z["k"]), L=int(z["L"]), parent=z["parent"], is_leaf=z["is_leaf"], desc=z["desc"],
                weight=z["weight"])
    return z, tree, np.ascontiguousarray(tree["desc"][z["query_node"]])


def flat_tree(seed: int, n: int = 65535, pairs=((100, 32767), (200, 32768), (32766, 50000), (32769, 50001),
                                                 (3, 65534))) -> dict:
    """Depth 1: n leaves under the root (65 535 is the most orbfe_vocab_create takes, the 16 low bits of the
    descent's key hold the child position), random descriptors, and for each (a, b) of pairs leaf b equal to
    leaf a, a < b: positions on both sides of 2^15, and the last position against lane 3."""
    rng = np.random.Generator(np.random.PCG64(seed))
    desc = rng.integers(0, 256, (n + 1, 32), dtype=np.uint8)
    desc[0] = 0
    for a, b in pairs:
        assert a < b < n
        desc[1 + b] = desc[1 + a]
    weight = np.concatenate([[0.0], rng.uniform(0.05, 6.0, n)])
    return dict(k=10, L=1, parent=np.zeros(n + 1, np.int32), is_leaf=np.concatenate([[0], np.ones(n)]).astype(np.uint8),
                desc=desc, weight=weight, pairs=tuple(pairs))


def flat_queries(tree: dict, seed: int):
    """64 copies of leaves (both members of every planted pair, the first and last positions, the positions
    around 2^15, random ones) and 32 more with 1..6 bits flipped, where the key's distance field is not zero.
    Returns (queries, child position each was taken from)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = len(tree["parent"]) - 1
    pos = [p for ab in tree["pairs"] for p in ab] + [0, 1, 31, 32, 33, 32766, 32769, n - 2, n - 1]
    pos = list(dict.fromkeys(pos))
    pos += rng.choice(n, 64 - len(pos), replace=False).tolist()
    copies = tree["desc"][1 + np.array(pos)]
    far = rng.integers(32768, n, 32)
    noisy = np.stack([flip_bits(rng, tree["desc"][1 + p], 1, 1 + i % 6)[0] for i, p in enumerate(far.tolist())])
    return np.ascontiguousarray(np.concatenate([copies, noisy])), np.concatenate([pos, far])


RAGGED = dict(seed=2, k=10, L=4, p_stop=0.25, p_dup=0.1, p_zero=0.1, order="dfs")   # = golden k10L4_ragged


def ragged_tree() -> dict:
    import vocab_synth as VS
    return VS.make_tree(**RAGGED)


def mismatched_tree(seed: int) -> dict:
    """The ragged tree with leaf flags that disagree with the children lists, as orbfe_vocab_create and the text
    format allow: 70 % of the nodes with children are flagged (they take a word id nobody can reach, which
    shifts every later word id) and 15 % of the childless nodes are unflagged and get a positive weight (the
    reference leaves their word_id at 0, TemplatedVocabulary.py:75-80, and still adds their weight)."""
    t = ragged_tree()
    rng = np.random.Generator(np.random.PCG64(seed))
    parent = t["parent"]
    n = len(parent)
    has_child = np.zeros(n, bool)
    has_child[parent[1:]] = True
    leaf = t["is_leaf"].copy()
    weight = t["weight"].copy()
    inner = np.flatnonzero(has_child)
    inner = inner[inner > 0]
    flagged = inner[rng.random(len(inner)) < 0.7]
    leaf[flagged] = 1
    weight[flagged] = rng.uniform(0.05, 6.0, len(flagged))
    childless = np.flatnonzero(~has_child)
    unflag = childless[rng.random(len(childless)) < 0.15]
    leaf[unflag] = 0
    weight[unflag] = rng.uniform(0.05, 6.0, len(unflag))
    return dict(t, is_leaf=leaf, weight=weight, flagged_inner=flagged, unflagged_childless=unflag)


def trace(tree: dict, queries: np.ndarray) -> list:
    """Per query the levels of its descent as (node, winning child position, distances to all children): an
    independent walk (first strict minimum, as the reference) that the CPU tests hold against VocabOracle."""
    parent = np.asarray(tree["parent"])
    order = np.argsort(parent[1:], kind="stable") + 1
    lo = np.searchsorted(parent[order], np.arange(len(parent)), "left")
    hi = np.searchsorted(parent[order], np.arange(len(parent)), "right")
    out = []
    for q in queries:
        node, levels = 0, []
        while hi[node] > lo[node]:
            ch = order[lo[node]:hi[node]]
            d = _POP8[tree["desc"][ch] ^ q].sum(axis=1)
            p = int(np.argmin(d))
            levels.append((node, p, d))
            node = int(ch[p])
        out.append((levels, node))
    return out


def categories(levels) -> tuple:
    """What a descent exercises of the pass loop, over all its levels:
      late   the winner sits at child position >= 32 (found in a second or later pass)
      cross  the minimum distance is shared with a child of another 32-child pass
      lower  ... with a child on a lower lane (position mod 32) than the winner's"""
    late = cross = lower = False
    for _, p, d in levels:
        eq = np.flatnonzero(d == d[p])
        late |= p >= 32
        cross |= bool(np.any(eq // 32 != p // 32))
        lower |= bool(np.any(eq % 32 < p % 32))
    return late, cross, lower


# ---- BoW vectors ------------------------------------------------------------------------------------------------
def kernel_constants() -> dict:
    """The constexpr ints of orbfe_kfdb.hip, read from its source text."""
    src = (ROOT / "pyorbslam_amd" / "csrc" / "orbfe_kfdb.hip").read_text()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (k\w+) = (\d+);", src)}


def random_vec(r, n: int, weights=None) -> OrderedDict:
    w = np.sort(r.choice(N_WORDS, n, replace=False))
    return with_weights(r, w, weights)


def with_weights(r, words, weights=None) -> OrderedDict:
    """Ascending word ids with L1-normalised weights in (0, 1), or with draws from the list `weights`."""
    words = np.asarray(words, np.int64)
    if weights is None:
        v = r.random(len(words)) + 0.05
        v = v / v.sum() if len(v) else v
    else:
        v = r.choice(np.asarray(weights, np.float64), len(words))
    return OrderedDict(zip(words.tolist(), v.tolist()))


def overlapping_vec(r, q: dict, n: int, share=0.5, weights=None) -> OrderedDict:
    """n distinct words, about `share` of them (as far as the query has that many) taken from the query q."""
    qk = np.fromiter(q.keys(), np.int64, len(q))
    k = min(int(round(n * share)), len(qk))
    if n and len(qk) and k == 0:
        k = 1
    mine = r.choice(qk, k, replace=False)
    other = np.setdiff1d(r.choice(N_WORDS, 2 * (n - k) + 16, replace=False), qk)
    r.shuffle(other)
    return with_weights(r, np.sort(np.concatenate([mine, other[: n - k]])), weights)


LONG_SLOTS = 8192 + 13
LONG_NQ = 200
LONG_KEEP = (8191, 8192, 8193, 8204)


def long_database(seed: int = 31):
    """(query, vectors, erased slot numbers).  8 205 vectors of lengths s % 71, about half of each vector's words
    taken from the 200-word query; slot 8 192 is the query itself.  A launch has kBowWaves * kBowMaxBlocks = 8 192
    waves, so the waves of slots 0..12 go on to slots 8 192..8 204 and all others stop after one."""
    r = np.random.default_rng(seed)
    q = random_vec(r, LONG_NQ)
    vecs = [overlapping_vec(r, q, s % 71) for s in range(LONG_SLOTS)]
    vecs[8192] = OrderedDict(q)
    erased = [s for s in np.flatnonzero(r.random(LONG_SLOTS) < 0.02).tolist() if s not in LONG_KEEP]
    return q, vecs, erased


PASS_LENGTHS = [255, 256, 257, 511, 512, 513, 1000]   # around the 64 * kBowUnroll = 256-word pass


def pass_world(nq: int, seed: int):
    """A query of nq words and one stored vector per PASS_LENGTHS entry sharing half its words with it, then
    the same lengths sharing every word they can."""
    r = np.random.default_rng(seed)
    q = random_vec(r, nq)
    return q, [overlapping_vec(r, q, n, share) for share in (0.5, 1.0) for n in PASS_LENGTHS]


SINGLE_POSITIONS = [0, 63, 64, 255, 256, 257, 511, 599]


def single_shared_world(seed: int = 41):
    """A 300-word query (multiples of 1000, among them 1000 * p for every p of SINGLE_POSITIONS) and per p a
    600-word stored vector 1000 * i + (1..999), i = 0..599, whose entry p is replaced by 1000 * p: the only
    multiple of 1000 it holds, so the one word it shares with the query, at stored position p."""
    r = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(1000), SINGLE_POSITIONS)
    qw = np.sort(np.concatenate([r.choice(rest, 300 - len(SINGLE_POSITIONS), replace=False), SINGLE_POSITIONS])) * 1000
    q = with_weights(r, qw)
    vecs = []
    for p in SINGLE_POSITIONS:
        w = 1000 * np.arange(600) + r.integers(1, 1000, 600)
        w[p] = 1000 * p
        vecs.append(with_weights(r, w))
    return q, vecs


EDGE_QUERY_LENGTHS = [2, 3, 8191, 8192, 8194]   # kBowLdsWords = 8192 is the last length staged in LDS


def extended_world(nq: int, seed: int):
    """world() of tests/test_kfdb_gpu.py (imported, not copied) plus stored vectors of the PASS_LENGTHS that
    share half their words with the query."""
    from test_kfdb_gpu import world
    q, vecs = world(N_WORDS, nq, seed)
    r = np.random.default_rng(seed + 1)
    return q, vecs + [overlapping_vec(r, q, n) for n in PASS_LENGTHS]


_MAGNITUDES = [0.0, 5e-324, 1e-310, 1e-300, 1.0, 1e300]
ODD_WEIGHTS = _MAGNITUDES + [-x for x in _MAGNITUDES]   # GeneralScoring.l1_score takes any Python floats


def odd_weight_world(seed: int = 51):
    """Zero, subnormal, huge and negative weights (no NaN, no inf) on a 300-word query and 48 stored vectors of
    1..600 words that share most words with it; then the query's words with other draws."""
    r = np.random.default_rng(seed)
    q = with_weights(r, np.sort(r.choice(N_WORDS, 300, replace=False)), ODD_WEIGHTS)
    lengths = [1, 2, 3, 63, 64, 65, 255, 256, 257, 600] + r.integers(1, 600, 37).tolist()
    vecs = [overlapping_vec(r, q, n, 0.8, ODD_WEIGHTS) for n in lengths]
    vecs.append(with_weights(r, list(q.keys()), ODD_WEIGHTS))
    # shared words whose weights are all zero or tiny on both sides: the terms and the score stay subnormal
    small = [x for x in ODD_WEIGHTS if abs(x) < 1e-300]
    quiet = [k for k, x in q.items() if abs(x) < 1e-300]
    for n in (1, 2, 3, 5, 8, 13, 21, len(quiet)):
        vecs.append(with_weights(r, np.sort(r.choice(quiet, n, replace=False)), small))
    return q, vecs
