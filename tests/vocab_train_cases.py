"""Named small training inputs for orbfe_vocab_train, and the implementation's tile constants the edge lengths
derive from.  A case is dict(frames=[(n_i, 32) uint8 ...], k, L, weighting, seed, max_iter); expected(name) trains
it with the definition (tests/vocab_train_definition.py), once per process.
"""
from __future__ import annotations

import numpy as np

import vocab_train_definition as VD

# pyorbslam_amd/csrc/orbfe_vocabtrain.hip
WAVE = 64       # lanes of a ballot (k_train_scatter's ranks, the scans of k_train_seed_pick)
THREADS = 256   # kTrainThreads: one tile of k_train_mean / k_train_scatter
CHUNK = 2048    # kTrainChunk: positions per workgroup; a longer node spans several workgroups and takes the
                # global bit counters and k_train_mean_final

EDGE_SIZES = sorted({WAVE - 1, WAVE, WAVE + 1, THREADS - 1, THREADS, THREADS + 1, CHUNK - 1, CHUNK, CHUNK + 1,
                     2 * CHUNK, 2 * CHUNK + 1})


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def noise(rng, n, ands=3):
    m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for _ in range(ands - 1):
        m &= rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return m


def clustered(seed, n, n_bases, ands=3):
    """n descriptors: random bases XOR a mask that is the AND of `ands` random bytes."""
    rng = _rng(seed)
    bases = rng.integers(0, 256, (n_bases, 32), dtype=np.uint8)
    return bases[rng.integers(0, n_bases, n)] ^ noise(rng, n, ands)


def cut_frames(D, n_frames, seed=0, empty=()):
    """D cut into n_frames images of random lengths in order; the images listed in `empty` get none."""
    rng = _rng(1000 + seed)
    full = [f for f in range(n_frames) if f not in set(empty)]
    cuts = np.sort(rng.integers(0, len(D) + 1, len(full) - 1))
    parts = np.split(D, cuts)
    out, it = [], iter(parts)
    for f in range(n_frames):
        out.append(np.zeros((0, 32), np.uint8) if f in set(empty) else next(it))
    return out


def case(D, k, L, n_frames=3, weighting=VD.TF_IDF, seed=0, max_iter=64, empty=()):
    return dict(frames=cut_frames(np.ascontiguousarray(D, np.uint8), n_frames, seed, empty), k=k, L=L,
                weighting=weighting, seed=seed, max_iter=max_iter)


def _one_bit(base, bit):
    d = base.copy()
    d[bit // 8] ^= 1 << (bit % 8)
    return d


def _many_small(seed=5):
    """Two levels of k = 18 over 18 x 18 tight groups of 2 .. 30 members: some 300 small nodes split at depth 2."""
    rng = _rng(seed)
    out = []
    for top in rng.integers(0, 256, (18, 32), dtype=np.uint8):
        for mid in top ^ noise(rng, 18, 2):
            n = int(rng.integers(2, 31))
            out.append(mid ^ noise(rng, n, 5))
    D = np.concatenate(out)
    return D[rng.permutation(len(D))]


def _big_beside_tiny(seed=6):
    """One tight group of 5 000 beside groups of 3, 5 and 12 that lie far from it and from each other."""
    rng = _rng(seed)
    bases = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    parts = [bases[0] ^ noise(rng, 5000, 6)] + [b ^ noise(rng, n, 6) for b, n in zip(bases[1:], (3, 5, 12))]
    D = np.concatenate(parts)
    return D[rng.permutation(len(D))]


def _nearly_identical(odd_at, n=12):
    """n - 1 copies of one descriptor and one that differs from it in one bit, at position odd_at: with centre 0 among
    the copies the seeding sees S = 1, so cut = 1 = S and the pick is that member (the first or the last)."""
    base = _rng(7).integers(0, 256, 32, dtype=np.uint8)
    D = np.repeat(base[None, :], n, axis=0)
    D[odd_at] = _one_bit(base, 77)
    return D


def _weights_data(empty=(2, 5)):
    """Four far groups (k = 4, L = 1 gives one word each): group 0 appears in every non-empty image, the others in
    some.  Without empty images Ni = n_frames for group 0's word: its weight is log(1) = 0.0 exactly."""
    rng = _rng(8)
    bases = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    frames = []
    for f in range(7):
        if f in empty:
            frames.append(np.zeros((0, 32), np.uint8))
            continue
        groups = [0, 0] + [g for g in (1, 2, 3) if (f + g) % 3 != 0]
        frames.append(np.concatenate([bases[g] ^ noise(rng, 3, 6) for g in groups]))
    return frames


def _build():
    c = {}
    r = _rng(1)
    rand = r.integers(0, 256, (64, 32), dtype=np.uint8)
    c["n1"] = case(rand[:1], 4, 2, n_frames=1)
    c["n2"] = case(rand[:2], 4, 2, n_frames=2)
    c["n_k"] = case(rand[:4], 4, 2)
    c["n_k_plus_1"] = case(rand[:5], 4, 2)
    c["identical"] = case(np.repeat(rand[:1], 30, axis=0), 4, 4)                # a chain of single children
    c["three_values_of_50"] = case(rand[_rng(2).integers(0, 3, 50)], 10, 2)      # S = 0 after three centres
    for n in EDGE_SIZES:
        c[f"node_{n}"] = case(clustered(100 + n, n, 7), 5, 2, seed=n)
    c["many_small"] = case(_many_small(), 18, 3, n_frames=9, seed=3)
    c["big_beside_tiny"] = case(_big_beside_tiny(), 4, 2, n_frames=5, seed=1)
    c["seeds_only"] = case(clustered(9, 700, 12), 6, 3, n_frames=4, seed=11, max_iter=1)
    c["cut_is_S_last"] = case(_nearly_identical(11), 4, 1, n_frames=1, seed=2, max_iter=1)
    c["cut_is_S_first"] = case(_nearly_identical(0), 4, 1, n_frames=1, seed=2, max_iter=1)
    c["capped_2"] = case(clustered(10, 900, 9), 5, 2, max_iter=2, seed=4)
    c["capped_3"] = case(clustered(10, 900, 9), 5, 2, max_iter=3, seed=4)
    c["k20_L1"] = case(clustered(11, 600, 30), 20, 1, n_frames=6, seed=5)
    c["L10_on_40"] = case(clustered(12, 40, 3, ands=2), 2, 10, seed=6)
    c["emptied_cluster"] = case(clustered(13, 312, 5), 9, 1, seed=7)
    for name, w in VD.WEIGHTINGS.items():
        c[f"weights_{name}"] = dict(frames=_weights_data(), k=4, L=1, weighting=w, seed=0, max_iter=64)
    c["weight_zero"] = dict(frames=_weights_data(empty=()), k=4, L=1, weighting=VD.TF_IDF, seed=0, max_iter=64)
    D = clustered(14, 500, 6)
    c["frames_cut_a"] = case(D, 4, 2, n_frames=3, seed=9)
    c["frames_cut_b"] = dict(c["frames_cut_a"], frames=cut_frames(D, 11, seed=77, empty=(4,)))
    return c


CASES = _build()
_EXPECTED: dict = {}


def expected(name, trace=None):
    """The definition's tree for a case (cached; a traced run is not)."""
    c = CASES[name]
    if trace is not None:
        return VD.train(c["frames"], c["k"], c["L"], c["weighting"], c["seed"], c["max_iter"], trace=trace)
    if name not in _EXPECTED:
        _EXPECTED[name] = VD.train(c["frames"], c["k"], c["L"], c["weighting"], c["seed"], c["max_iter"])
    return _EXPECTED[name]


def medium():
    """About 20 000 clustered descriptors in 40 images: 200 random bases XOR the AND of three random bytes."""
    return case(clustered(20, 20000, 200), 10, 3, n_frames=40, seed=0)
