"""What k_fuse_search buys: fuse_pkf_mp for all the neighbours of a new keyframe in one launch.

LocalMapping.search_in_neighbors calls ORBMatcher.fuse_pkf_mp once per target keyframe with the current keyframe's
map points, and once more for the current keyframe with the targets' pooled points.  This compares that loop of N
single calls (one k_hamming_search launch, a Python projection and a Python replay each; still in the tree, so it is
the baseline) with one fuse_pkf_mp_many call, N in --neigh, and the pooled call both ways.  Fusing changes the map,
so every sample runs on a fresh build of the same tests/matcher_world world of `--feats` features per keyframe.
make_world's own world only adds observations (every re-observed feature's slot is empty or holds the same point);
with --clones a share of the neighbours' slots holds a clone of the point they re-observe
(tests/fuse_cases.clone_world), so that points get replaced as well: MapPoint.replace and its descriptor
recomputation then run inside both variants, and the survivors' changed descriptors send items of later keyframes
through the single-item path.  Beside the many call: its kernel time (orbfe_fuse_search_last_ms), the time of
packing keyframes and points into arrays on a fresh build, and the share of items that came back marginal.

Every measurement is taken --rounds times, the variants alternating inside a round; the JSON holds every sample.
--many-only runs the many call alone (the shape to put under a kernel trace).

  python tools/bench_fuse.py [--rounds 3] [--neigh 1 10 30] [--feats 2000] [--clones] [--out FILE]
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

TH = 3.0


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4),
            "samples": [round(x, 4) for x in xs]}


def fresh(z):
    import matcher_world as MW
    w = MW.build(z)
    w.mp_id = lambda mp: -1 if mp is None else mp.mnId  # the stand-in's linear search would be in every timing
    return w


def shape(w, n, pooled):
    """(keyframes, points) of one call on a fresh world."""
    import fuse_cases as FC
    if pooled:
        return [w.kfs[0]], FC.pooled_points(w.kfs[1:1 + n])
    return w.kfs[1:1 + n], w.kfs[0].get_map_point_matches()


def run(a):
    import fuse_cases as FC
    from pyorbslam_amd import _lib, matcher
    n_max = max(a.neigh)
    import matcher_world as MW
    if a.clones:
        z = FC.Z(FC.clone_world(13, n_kf=n_max + 1, n=a.feats, n_mp=int(a.feats * 0.7)))
    else:
        z = FC.Z(MW.make_world(np.random.Generator(np.random.PCG64(13)), n_kf=n_max + 1, n=a.feats,
                               n_mp=int(a.feats * 0.7)))
    m = matcher.ORBMatcher()
    seen = []
    arrays = matcher.fuse_search_arrays
    matcher.fuse_search_arrays = lambda *x, **k: seen.append(arrays(*x, **k)) or seen[-1]
    out = {"features": a.feats, "world": "clone_world" if a.clones else "make_world"}
    for n, pooled in [(n, False) for n in a.neigh] + [(n_max, True)]:
        # warm-up of both, and the equality of what they return
        w = fresh(z)
        kfs, pts = shape(w, n, pooled)
        got = m.fuse_pkf_mp_many(kfs, pts, TH)
        if not a.many_only:
            w = fresh(z)
            kfs, pts = shape(w, n, pooled)
            assert got == [m.fuse_pkf_mp(kf, pts, TH) for kf in kfs]
        loop, many, pack, kern, marg = [], [], [], [], []
        for _ in range(a.rounds):
            if not a.many_only:
                w = fresh(z)
                kfs, pts = shape(w, n, pooled)
                t0 = time.perf_counter()
                for kf in kfs:
                    m.fuse_pkf_mp(kf, pts, TH)
                loop.append((time.perf_counter() - t0) * 1e3)
            w = fresh(z)
            kfs, pts = shape(w, n, pooled)
            del seen[:]
            t0 = time.perf_counter()
            m.fuse_pkf_mp_many(kfs, pts, TH)
            many.append((time.perf_counter() - t0) * 1e3)
            ms = C.c_float()
            _lib.call("orbfe_fuse_search_last_ms", C.byref(ms))
            kern.append(ms.value)
            st = seen[0]["status"]
            marg.append(float(np.count_nonzero(st)) / max(st.size, 1))
            w = fresh(z)
            kfs, pts = shape(w, n, pooled)
            t0 = time.perf_counter()
            for kf in kfs:
                matcher._fuse_frame(kf)
            for p in pts:
                if p and not p.is_bad():
                    matcher._fuse_point(p)
            pack.append((time.perf_counter() - t0) * 1e3)
        key = f"pooled_{n}" if pooled else str(n)
        w = fresh(z)
        kfs, pts = shape(w, n, pooled)
        m.fuse_pkf_mp_many(kfs, pts, TH)
        n_replace = sum(1 for e in w.log if e[0] == MW.EV_REPLACE)
        out[key] = {"replace_events": n_replace,
                    "keyframes": len(kfs), "points": len(pts), "items": int(seen[0]["status"].size),
                    "many_ms": spread(many), "many_packing_ms": spread(pack), "many_kernel_ms": spread(kern),
                    "marginal_share_of_items": spread(marg), "fused": [int(g) for g in got]}
        if not a.many_only:
            out[key]["loop_ms"] = spread(loop)
            out[key]["every_many_sample_below_every_loop_sample"] = max(many) < min(loop)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--neigh", type=int, nargs="+", default=[1, 10, 30])
    ap.add_argument("--feats", type=int, default=2000)
    ap.add_argument("--many-only", action="store_true")
    ap.add_argument("--clones", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"metric": "fuse_pkf_mp, many keyframes per launch (k_fuse_search)", "rounds": a.rounds,
           "many_vs_loop": run(a)}
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
