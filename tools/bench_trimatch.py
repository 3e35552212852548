"""What k_tri_match buys: search_for_triangulation for all the neighbours of a new keyframe in one launch.

LocalMapping.create_new_map_points calls ORBMatcher.search_for_triangulation once per covisible neighbour.  This
compares that loop of N single searches (one k_hamming_search launch and a Python replay each; still in the tree,
so it is the baseline) with one search_for_triangulation_many call, on a tests/matcher_world world of `--feats`
features per keyframe in LocalMapping's shape (most features of every keyframe without a map point,
ORBMatcher(0.6, False)), N in --cands.  The many call's object-to-array conversion and its kernel time
(orbfe_tri_match_last_ms) are reported beside it.

Every measurement is taken --rounds times, the variants alternating inside a round; the JSON holds every sample.
--many-only runs the many call alone (the shape to put under a kernel trace).

  python tools/bench_trimatch.py [--rounds 3] [--cands 1 4 10] [--feats 2000] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


class _Z:
    def __init__(self, d):
        self._d, self.files = d, list(d.keys())

    def __getitem__(self, k):
        return self._d[k]


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4),
            "samples": [round(x, 4) for x in xs]}


def make_world(a):
    import matcher_world as MW
    rng = np.random.Generator(np.random.PCG64(13))
    n_max = max(a.cands)
    z = MW.make_world(rng, n_kf=n_max + 1, n=a.feats, n_mp=int(a.feats * 0.7), n_words=a.feats // 15)
    for j in range(n_max + 1):  # a fresh keyframe and its neighbours hold map points in a minority of their slots
        z[f"kfmp{j}"] = np.where(rng.random(a.feats) < 0.8, -1, z[f"kfmp{j}"]).astype(np.int32)
    w = MW.build(_Z(z))
    return w, [MW.fundamental(w.kfs[0], kf) for kf in w.kfs[1:]]


def run(a):
    from pyorbslam_amd import _lib, matcher
    w, F = make_world(a)
    m = matcher.ORBMatcher(0.6, False)
    k0 = w.kfs[0]
    free = [sum(1 for p in kf.mvpMapPoints if not p) for kf in w.kfs]
    out = {"features": a.feats, "free_slots_keyframe0": free[0]}
    for n in a.cands:
        kfs, Fs = w.kfs[1:1 + n], F[:n]
        got = m.search_for_triangulation_many(k0, kfs, Fs)  # warm-up of both, and one result
        if not a.many_only:
            assert got == [m.search_for_triangulation(k0, kf, f) for kf, f in zip(kfs, Fs)]
        loop, many, conv, kern = [], [], [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            if not a.many_only:
                for kf, f in zip(kfs, Fs):
                    m.search_for_triangulation(k0, kf, f)
            t1 = time.perf_counter()
            m.search_for_triangulation_many(k0, kfs, Fs)
            t2 = time.perf_counter()
            ms = C.c_float()
            _lib.call("orbfe_tri_match_last_ms", C.byref(ms))
            for kf in [k0] + kfs:
                matcher._tri_frame(kf)
            t3 = time.perf_counter()
            loop.append((t1 - t0) * 1e3)
            many.append((t2 - t1) * 1e3)
            conv.append((t3 - t2) * 1e3)
            kern.append(ms.value)
        out[str(n)] = {"many_ms": spread(many), "many_object_to_array_ms": spread(conv),
                       "many_kernel_ms": spread(kern), "matches": [len(g) for g in got]}
        if not a.many_only:
            out[str(n)]["loop_ms"] = spread(loop)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cands", type=int, nargs="+", default=[1, 4, 10])
    ap.add_argument("--feats", type=int, default=2000)
    ap.add_argument("--many-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"metric": "search_for_triangulation, many neighbours per launch (k_tri_match)", "rounds": a.rounds,
           "many_vs_loop": run(a)}
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
