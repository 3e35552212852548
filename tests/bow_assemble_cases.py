"""Inputs of tests/test_gpu_bow_assemble.py (k_bow_assemble: BoW and feature vectors assembled on the device) and
the facts tests/test_bow_assemble_cases_cpu.py checks about them.  Everything here is computed with VocabOracle
alone (its own transform, with the descents of a frame pool memoised), so the CPU test can show that each case
contains what it is for and the GPU test cannot pass vacuously.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

import vocab_synth as VS
from oracle.vocab_oracle import VocabOracle

ROOT = Path(__file__).resolve().parents[1]

# The kernel's geometry, restated (test_bow_assemble_cases_cpu.py holds it against the sources): a frame of up to
# 2 048 features takes a 256-thread workgroup, a longer one a 1 024-thread workgroup; the bitonic sort pads the kept
# features to the next power of two, at least 2.
MAX_FRAME = 8192
SMALL_FRAME = 2048
WORKGROUPS = (256, 1024)
ITEMS = 8
ISSUE_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]
PADDED = [2 ** k for k in range(1, 14)]                    # 2 .. 8 192: the sort's padded sizes
EDGE_LENGTHS = sorted({n for p in list(WORKGROUPS) + PADDED + [SMALL_FRAME] for n in (p - 1, p, p + 1)
                       if 0 <= n <= MAX_FRAME} | set(ISSUE_LENGTHS) | {MAX_FRAME})


def source_constants() -> dict:
    """ORBFE_BOW_MAX_FRAME of the header and the constexpr ints of orbfe_vocab.hip, read from the source text."""
    src = (ROOT / "pyorbslam_amd" / "csrc" / "orbfe_vocab.hip").read_text()
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (k\w+) = (\d+);", src)}
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    out["ORBFE_BOW_MAX_FRAME"] = int(re.search(r"#define ORBFE_BOW_MAX_FRAME (\d+)", hdr).group(1))
    return out


class PoolOracle(VocabOracle):
    """VocabOracle whose descents are remembered per (descriptor, level): the frames below draw from a pool with
    replacement, and transform() (the parent's, unchanged) descends every feature."""

    def __init__(self, tree):
        super().__init__(tree["parent"], tree["is_leaf"], tree["desc"], tree["weight"], tree["L"])
        self._memo = {}

    def descend(self, q, nid_level):
        key = (bytes(q), nid_level)
        r = self._memo.get(key)
        if r is None:
            r = self._memo[key] = super().descend(q, nid_level)
        return r


def small_tree() -> dict:
    """Ragged (descents stop above the node level), zero-weight leaves, equal children, 4 to 64 words: a frame of
    any length is mostly duplicates."""
    return VS.make_tree(seed=30, k=4, L=3, p_stop=0.3, p_dup=0.2, p_zero=0.15, order="dfs")


def wide_tree() -> dict:
    """8 000 words, every weight positive (a frame's kept features are all its features, so the frame lengths are
    the sort's sizes exactly), few duplicates per frame."""
    return VS.make_tree(seed=32, k=20, L=3, p_zero=0.0)


def patched_tree():
    """small_tree() with the weight of one reachable leaf negative and of another NaN.  Returns (tree, negative
    node, NaN node)."""
    t = small_tree()
    o = PoolOracle(t)
    pool = VS.query_descriptors(t, 33, 400)
    leaves = np.flatnonzero(t["is_leaf"] > 0)   # word id -> node (make_tree flags exactly the childless nodes)
    hit = []
    for q in pool:
        word, _, w = o.descend(q, 0)
        if w > 0 and int(leaves[word]) not in hit:
            hit.append(int(leaves[word]))
    t["weight"] = t["weight"].copy()
    t["weight"][hit[0]] = -1.5
    t["weight"][hit[1]] = np.nan
    return t, hit[0], hit[1]


LEVELS_UP = 1   # node level L - 1 = 2: a descent that ends at depth 1 has no node of its own


def length_frames(tree: dict, seed: int, pool_size: int) -> list:
    """One frame per EDGE_LENGTHS entry, drawn with replacement from a seeded pool, with empty frames first, last
    and in the middle.  The longest frames come first among the rest so that short frames follow long ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = VS.query_descriptors(tree, seed + 1, pool_size)
    lengths = [n for n in EDGE_LENGTHS if n > 0]
    lengths = lengths[::-1]
    lengths = [0] + lengths[:len(lengths) // 2] + [0] + lengths[len(lengths) // 2:] + [0]
    return [pool[rng.integers(0, len(pool), n)] for n in lengths]


def special_frames(tree: dict, o: VocabOracle, seed: int) -> dict:
    """Named frames on a ragged tree with zero weights, in launch order (dict order):
      ends_valid     ends with a feature that has a node of its own
      starts_short   starts with two descents that stop above the node level (they take node 0, not the node
                     the previous frame ended with), then valid ones
      long_run       70 features of one word between others
      one_word       300 features, all of one word: the run crosses lanes, waves and the 256-thread workgroup
      holes          kept and dropped features alternating
      all_dropped    only zero-weight features
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = VS.query_descriptors(tree, seed + 1, 900)
    d = [o.descend(q, o.L - LEVELS_UP) for q in pool]
    valid = [i for i, (_, n, w) in enumerate(d) if n >= 0 and w > 0]
    short = [i for i, (_, n, w) in enumerate(d) if n < 0 and w > 0]
    zero = [i for i, (_, n, w) in enumerate(d) if not w > 0]
    kept = [i for i, (_, n, w) in enumerate(d) if w > 0]
    by_word = {}
    for i in kept:
        by_word.setdefault(d[i][0], []).append(i)
    same = max(by_word.values(), key=len)    # descriptors of the most frequent word

    def draw(idx, n):
        return [idx[int(j)] for j in rng.integers(0, len(idx), n)]

    frames = dict(
        ends_valid=draw(kept, 40) + [valid[0]],
        starts_short=[short[0], short[1 % len(short)]] + draw(valid, 3) + draw(kept, 60),
        long_run=draw(kept, 90) + draw(same, 70) + draw(kept, 100),
        one_word=draw(same, 300),
        holes=[i for pair in zip(draw(kept, 150), draw(zero, 150)) for i in pair],
        all_dropped=draw(zero, 77),
    )
    f = frames["long_run"]
    frames["long_run"] = [f[int(j)] for j in rng.permutation(len(f))]
    return {k: pool[np.array(v, np.int64)] for k, v in frames.items()}


def arrays_of(result):
    """An oracle (BowVector, FeatureVector) as the kernel's arrays: word, weight bits, node, end, idx, n_kept."""
    bv, fv = result
    lens = [len(v) for v in fv.values()]
    return (np.array(list(bv.keys()), np.int32), np.array(list(bv.values()), np.float64).view(np.uint64),
            np.array(list(fv.keys()), np.int32), np.cumsum(lens).astype(np.int32),
            np.array([i for v in fv.values() for i in v], np.int32), int(sum(lens)))


def assert_arrays(got, want, what=""):
    """A BowArrays against an oracle result, exactly: ids, f64 bit patterns, CSR ends, indices, n_kept."""
    w = arrays_of(want)
    g = (got.word, np.ascontiguousarray(got.weight).view(np.uint64), got.node, got.end, got.idx, got.n_kept)
    for name, a, b in zip(("word", "weight bits", "node", "end", "idx"), g, w):
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: {name} differs"
    assert g[5] == w[5], f"{what}: n_kept {g[5]} != {w[5]}"
