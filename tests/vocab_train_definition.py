"""The definition of vocabulary training (orbfe_vocab_train), restated in plain NumPy / Python.

DBoW2's HKmeansStep / initiateClustersKMpp / setNodeWeights built level by level, with every choice it leaves open
fixed ("Training a vocabulary").  Integer only, so an implementation is compared bit for bit.
train() returns the node arrays of TemplatedVocabulary.node_arrays() and the counters of train_stats().
"""
from __future__ import annotations

import math

import numpy as np

MASK = (1 << 64) - 1
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
WEIGHTINGS = {"TF_IDF": TF_IDF, "TF": TF, "IDF": IDF, "BINARY": BINARY}
MAX_L = 10

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def splitmix64(z: int) -> int:
    z &= MASK
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & MASK
    z ^= z >> 31
    return z


def draw(seed: int, node: int, j: int) -> int:
    return splitmix64(seed + (32 * node + j + 1) * 0x9E3779B97F4A7C15)


def distance(a, b) -> int:
    """FORB.distance."""
    return int(_POP[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum())


def distances(descs, centre) -> np.ndarray:
    return _POP[np.bitwise_xor(descs, centre[None, :])].sum(axis=1)


def mean_value(descs) -> np.ndarray:
    """FORB.meanValue: bit b is set iff count_b >= n // 2 + n % 2."""
    descs = np.asarray(descs, np.uint8).reshape(-1, 32)
    n = len(descs)
    counts = np.unpackbits(descs, axis=1).astype(np.int64).sum(axis=0)
    return np.packbits(counts >= n // 2 + n % 2)


def seed_centres(D, members, node, k, seed, trace=None):
    """Integer kmeans++: the member ranks of the chosen centres (fewer than k when S reaches 0)."""
    n = len(members)
    X = D[members]
    picks = [draw(seed, node, 0) % n]
    md = None
    for j in range(1, k):
        d = distances(X, X[picks[-1]])
        md = d if md is None else np.minimum(md, d)
        S = int(md.sum())
        if S == 0:
            break
        cut = 1 + draw(seed, node, j) % S
        run = np.cumsum(md)
        r = int(np.searchsorted(run, cut, side="left"))  # the first member whose running sum is >= cut
        if trace is not None:
            trace.append(dict(node=node, j=j, S=S, cut=cut, pick=r, n=n, exact=bool(run[r] == cut)))
        picks.append(r)
    return picks


def assign(X, centres):
    d = np.stack([distances(X, c) for c in centres], axis=1)
    return d.argmin(axis=1), d  # argmin: the lowest cluster index on ties


def split(D, members, node, k, seed, max_iter, info):
    """Clusters of one node: [(centre, members)] for the clusters that end with members, in cluster order."""
    n = len(members)
    if n <= k:
        return [(D[m].copy(), members[i:i + 1]) for i, m in enumerate(members)]
    X = D[members]
    picks = seed_centres(D, members, node, k, seed, info.get("trace"))
    centres = [X[r].copy() for r in picks]
    if len(centres) < k:
        info["short_seeded"] += 1
    prev, it = None, 0
    while True:
        it += 1
        if it > 1:
            for c in range(len(centres)):
                mem = X[prev == c]
                if len(mem):
                    counts = np.unpackbits(mem, axis=1).astype(np.int64).sum(axis=0)
                    if np.any(counts * 2 == len(mem)):
                        info["exact_half"] += 1
                    centres[c] = mean_value(mem)
        cur, d = assign(X, centres)
        srt = np.sort(d, axis=1)
        if d.shape[1] > 1 and np.any(srt[:, 0] == srt[:, 1]):
            info["ties"] += 1
        if prev is not None and np.array_equal(cur, prev):
            break
        prev = cur
        if it == max_iter:
            info["capped"] += 1
            break
    info["iter_sum"] += it
    info["iter_max"] = max(info["iter_max"], it)
    out = []
    for c in range(len(centres)):
        mem = members[cur == c]
        if len(mem):
            out.append((centres[c], mem))
        else:
            info["empty_dropped"] += 1
    return out


def descend(tree, q):
    """The existing descent: the child at the smallest distance, the first on ties, down to a node without
    children.  Returns the node reached by every descriptor of q."""
    parent = tree["parent"]
    n = len(parent)
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        kids[parent[i]].append(i)
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    at = np.zeros(len(q), np.int64)
    for node in range(n):  # parents come before their children
        if not kids[node]:
            continue
        idx = np.flatnonzero(at == node)
        if len(idx):
            d = np.stack([distances(q[idx], tree["desc"][c]) for c in kids[node]], axis=1)
            at[idx] = np.array(kids[node])[d.argmin(axis=1)]
    return at


def train(frames, k, L, weighting=TF_IDF, seed=0, max_iter=64, trace=None):
    frames = [np.asarray(f, np.uint8).reshape(-1, 32) for f in frames]
    n_frames = len(frames)
    assert n_frames >= 1
    D = np.concatenate(frames) if frames else np.zeros((0, 32), np.uint8)
    N = len(D)
    frame_of = np.repeat(np.arange(n_frames), [len(f) for f in frames])
    parent, desc, depth_of, members_of = [0], [np.zeros(32, np.uint8)], [0], [N]
    keys = ("nodes_split", "iter_sum", "iter_max", "capped", "empty_dropped", "short_seeded", "ties", "exact_half")
    stats = {key: [0] * MAX_L for key in keys}
    stats["single_above_L"] = 0
    level = [(0, np.arange(N))] if N >= 1 else []
    for depth in range(L):
        info = {key: 0 for key in keys}
        if trace is not None:
            info["trace"] = trace
        nxt = []
        for node, members in level:  # ascending node id
            info["nodes_split"] += 1
            for centre, mem in split(D, members, node, k, seed, max_iter, info):
                cid = len(parent)
                parent.append(node)
                desc.append(centre)
                depth_of.append(depth + 1)
                members_of.append(len(mem))
                if len(mem) > 1 and depth + 1 < L:
                    nxt.append((cid, mem))
                elif len(mem) == 1 and depth + 1 < L:
                    stats["single_above_L"] += 1
        for key in keys:
            stats[key][depth] = info[key]
        level = nxt
        if not level:
            break
    n = len(parent)
    parent = np.array(parent, np.int32)
    is_leaf = np.ones(n, np.uint8)
    is_leaf[parent[1:]] = 0
    is_leaf[0] = 0
    word_id = np.zeros(n, np.int32)
    word_id[is_leaf > 0] = np.arange(int(is_leaf.sum()))
    tree = dict(k=k, L=L, parent=parent, is_leaf=is_leaf, desc=np.stack(desc).astype(np.uint8), word_id=word_id)
    weight = np.zeros(n, np.float64)
    if weighting in (TF, BINARY):
        weight[is_leaf > 0] = 1.0
    elif N:
        reached = descend(tree, D)
        for node in np.flatnonzero(is_leaf):
            ni = len(set(frame_of[reached == node].tolist()))
            weight[node] = math.log(n_frames / ni) if ni > 0 else 0.0
    tree["weight"] = weight
    tree["depth_of"] = np.array(depth_of, np.int32)     # for the tests: a node's depth and its number of members
    tree["members"] = np.array(members_of, np.int64)
    stats.update(n_desc=N, n_nodes=n, n_words=int(is_leaf.sum()))
    tree["stats"] = stats
    return tree
