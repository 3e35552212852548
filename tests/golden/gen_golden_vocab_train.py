"""Generate the vocabulary-training goldens from the REFERENCE pyDBoW (build container only).

Records, in tests/golden/vocab_train_ref.npz:
  - FORB.meanValue of groups of 1, 2, 3, 4, 5, 8 and 9 descriptors (exact-half bit counts included) and
    FORB.distance spot values;
  - two trees trained by the definition (tests/vocab_train_definition.py) and written by the drop-in's
    save_to_text_file (host only), as the bytes of the text file;
  - per tree what the reference's own load_from_text_file + transform return for 200 queries at two levels_up.
Nothing here runs on the GPU box.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_vocab_train.py
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[2]
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, "/root/reference")

import vocab_train_cases as TC  # noqa: E402
import vocab_train_definition as VD  # noqa: E402
from pyDBoW.FORB import FORB  # noqa: E402
from pyDBoW.TemplatedVocabulary import TemplatedVocabulary as RefVocabulary  # noqa: E402

GROUPS = (1, 2, 3, 4, 5, 8, 9)
LEVELS_UP = {"k3L3": (1, 2), "k5L2_dup": (0, 1)}


def golden_trees():
    """name -> training case.  k3L3: about 150 clustered descriptors in 12 images; k5L2_dup: duplicates."""
    D = TC.clustered(31, 150, 7)
    dup = TC.clustered(32, 40, 4)
    dup = np.concatenate([dup, dup[:25], dup[:10]])
    return {"k3L3": TC.case(D, 3, 3, n_frames=12, seed=21),
            "k5L2_dup": TC.case(dup[TC._rng(33).permutation(len(dup))], 5, 2, n_frames=5, seed=22)}


def queries(c, seed, n=200):
    """Training descriptors, perturbed ones and noise."""
    rng = TC._rng(seed)
    D = np.concatenate(c["frames"])
    a = D[rng.integers(0, len(D), n // 2)]
    b = D[rng.integers(0, len(D), n // 4)] ^ TC.noise(rng, n // 4, 3)
    q = np.concatenate([a, b, rng.integers(0, 256, (n - len(a) - len(b), 32), dtype=np.uint8)])
    return q[rng.permutation(n)]


def main():
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    forb = FORB(32)
    out = {}
    rng = TC._rng(30)
    for n in GROUPS:
        g = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if n % 2 == 0:  # exact halves: the first half of the group is the complement of the second in byte 0 .. 15
            g[:n // 2, :16] = ~g[n // 2:, :16]
        out[f"mean_in_{n}"] = g
        out[f"mean_out_{n}"] = np.asarray(forb.meanValue(list(g)), np.uint8)
    pairs = rng.integers(0, 256, (40, 2, 32), dtype=np.uint8)
    pairs[0, 1] = pairs[0, 0]
    pairs[1, 1] = ~pairs[1, 0]
    out["dist_in"] = pairs
    out["dist_out"] = np.array([forb.distance(a, b) for a, b in pairs], np.int64)
    for i, (name, c) in enumerate(golden_trees().items()):
        t = VD.train(c["frames"], c["k"], c["L"], c["weighting"], c["seed"], c["max_iter"])
        q = queries(c, 40 + i)
        with tempfile.TemporaryDirectory() as td:
            path = Path(td) / "voc.txt"
            TemplatedVocabulary(c["k"], c["L"]).from_arrays(t["parent"], t["is_leaf"], t["desc"],
                                                            t["weight"]).save_to_text_file(path)
            out[f"{name}_text"] = np.frombuffer(path.read_bytes(), np.uint8)
            ref = RefVocabulary()
            assert ref.load_from_text_file(str(path))
        out[f"{name}_queries"] = q
        out[f"{name}_size"] = len(ref.words)
        for lu in LEVELS_UP[name]:
            bv, fv = ref.transform(q, lu)
            out[f"{name}_bv_word_{lu}"] = np.array(list(bv.keys()), np.int64)
            out[f"{name}_bv_w_{lu}"] = np.array(list(bv.values()), np.float64)
            out[f"{name}_fv_node_{lu}"] = np.array(list(fv.keys()), np.int64)
            out[f"{name}_fv_len_{lu}"] = np.array([len(v) for v in fv.values()], np.int64)
            out[f"{name}_fv_idx_{lu}"] = np.array([x for v in fv.values() for x in v], np.int64)
            print(name, "levels_up", lu, "nodes", len(t["parent"]), "words", len(bv), "fv nodes", len(fv))
    np.savez_compressed(GOLD / "vocab_train_ref.npz", **out)
    print((GOLD / "vocab_train_ref.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
