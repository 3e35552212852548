"""What k_sim3_search buys: LoopClosing.compute_sim3's mutual search, ORBMatcher.search_by_sim3, from one launch.

Single call: the host body (_sim3_host, the former body of the public method, so it is the baseline) against the
public method on a tests/matcher_world world of P features per keyframe, P in --feats, th = 7.5; s12 = 1.1, R12 and
t12 from the two poses with a small seeded perturbation of t12, a quarter of vpMatches12 pre-filled
(tests/sim3_cases.py).

Many: search_by_sim3_many over M candidates, M in --cands, against the loop of M public single calls on a world of
--many-feats features per keyframe; the many form packs pKF1 and sends its points once.

The search writes into vpMatches12, so every sample runs on a fresh build of the same world.  Beside each new call:
its kernel time (orbfe_sim3_search_last_ms), the time of packing keyframes and points into arrays on a fresh build,
and the share of items that came back marginal.  Every measurement is taken --rounds times, the variants alternating
inside a round; the JSON holds every sample.  --new-only runs the new calls alone (the shape to put under a kernel
trace).

  python tools/bench_sim3.py [--rounds 3] [--feats 2000 8000] [--cands 1 4 16] [--many-feats 2000] [--out FILE]
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

TH = 7.5


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4),
            "samples": [round(x, 4) for x in xs]}


def fresh(z):
    import matcher_world as MW
    w = MW.build(z)
    w.mp_id = lambda mp: -1 if mp is None else mp.mnId  # the stand-in's linear search would be in every timing
    return w


def last_ms():
    from pyorbslam_amd import _lib
    ms = C.c_float()
    _lib.call("orbfe_sim3_search_last_ms", C.byref(ms))
    return ms.value


def world(n_kf, feats, seed):
    import fuse_cases as FC
    import matcher_world as MW
    import sim3_cases as SC
    z = MW.make_world(np.random.Generator(np.random.PCG64(seed)), n_kf=n_kf, n=feats, n_mp=int(feats * 0.7))
    z.update(SC.make_sim3s(fresh(FC.Z(z)), seed + 1))
    return FC.Z(z)


def shape(z, n):
    """(pKF1, the five columns of n candidates) on a fresh build."""
    import sim3_cases as SC
    w = fresh(z)
    prs = SC.pairs_of(w, z, n)
    return w.kfs[0], [[p[c] for p in prs] for c in range(5)]


def encode(res):
    return [(int(n), [-1 if p is None else p.mnId for p in v]) for n, v in res]


def packing(m, kf1, cols):
    """What the device path does before its launch, without the launch."""
    from pyorbslam_amd import matcher
    t0 = time.perf_counter()
    matcher._fuse_frame(kf1)
    skip = lambda p: not p or p.is_bad()  # noqa: E731
    m._search_points(kf1.get_map_point_matches(), skip)
    for kf2, vm, s, R, t in zip(*cols):
        pp = m._sim3_prep(kf1.N, kf2, vm, s, R, t)
        m._search_points(pp[1], skip)
    return (time.perf_counter() - t0) * 1e3


def run_single(a, seen):
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    out = {}
    for P in a.feats:
        z = world(2, P, 17)
        kf1, cols = shape(z, 1)
        got = encode([m.search_by_sim3(kf1, *[c[0] for c in cols], TH)])
        if not a.new_only:
            kf1, cols = shape(z, 1)
            assert got == encode([m._sim3_host(kf1, *[c[0] for c in cols], TH)])
        host, dev, pack, kern, marg = [], [], [], [], []
        for _ in range(a.rounds):
            if not a.new_only:
                kf1, cols = shape(z, 1)
                t0 = time.perf_counter()
                m._sim3_host(kf1, *[c[0] for c in cols], TH)
                host.append((time.perf_counter() - t0) * 1e3)
            kf1, cols = shape(z, 1)
            del seen[:]
            t0 = time.perf_counter()
            m.search_by_sim3(kf1, *[c[0] for c in cols], TH)
            dev.append((time.perf_counter() - t0) * 1e3)
            kern.append(last_ms())
            st = seen[0]["status"]
            marg.append(float(np.count_nonzero(st)) / max(st.size, 1))
            pack.append(packing(m, *shape(z, 1)))
        out[str(P)] = {"features": P, "items": int(seen[0]["status"].size), "matches": got[0][0],
                       "prefilled": sum(1 for v in got[0][1] if v >= 0) - got[0][0], "device_ms": spread(dev),
                       "device_packing_ms": spread(pack), "device_kernel_ms": spread(kern),
                       "marginal_share_of_items": spread(marg)}
        if not a.new_only:
            out[str(P)]["host_ms"] = spread(host)
            out[str(P)]["every_new_sample_below_every_baseline_sample"] = max(dev) < min(host)
        print(f"single {P}: done", file=sys.stderr, flush=True)
    return out


def run_many(a, seen):
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    z = world(max(a.cands) + 1, a.many_feats, 13)
    out = {"features": a.many_feats}
    for n in a.cands:
        kf1, cols = shape(z, n)
        got = encode(m.search_by_sim3_many(kf1, *cols, TH))
        if not a.new_only:
            kf1, cols = shape(z, n)
            assert got == encode([m.search_by_sim3(kf1, *x, TH) for x in zip(*cols)])
        loop, many, pack, kern, marg = [], [], [], [], []
        for _ in range(a.rounds):
            if not a.new_only:
                kf1, cols = shape(z, n)
                t0 = time.perf_counter()
                for x in zip(*cols):
                    m.search_by_sim3(kf1, *x, TH)
                loop.append((time.perf_counter() - t0) * 1e3)
            kf1, cols = shape(z, n)
            del seen[:]
            t0 = time.perf_counter()
            m.search_by_sim3_many(kf1, *cols, TH)
            many.append((time.perf_counter() - t0) * 1e3)
            kern.append(last_ms())
            st = seen[0]["status"]
            marg.append(float(np.count_nonzero(st)) / max(st.size, 1))
            pack.append(packing(m, *shape(z, n)))
        out[str(n)] = {"candidates": n, "items": int(seen[0]["status"].size), "matches": [g[0] for g in got],
                       "many_ms": spread(many), "many_packing_ms": spread(pack), "many_kernel_ms": spread(kern),
                       "marginal_share_of_items": spread(marg)}
        if not a.new_only:
            out[str(n)]["loop_ms"] = spread(loop)
            out[str(n)]["every_new_sample_below_every_baseline_sample"] = max(many) < min(loop)
        print(f"many {n}: done", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--feats", type=int, nargs="*", default=[2000, 8000])
    ap.add_argument("--cands", type=int, nargs="*", default=[1, 4, 16])
    ap.add_argument("--many-feats", type=int, default=2000)
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pyorbslam_amd import matcher
    seen = []
    arrays = matcher.sim3_search_arrays
    matcher.sim3_search_arrays = lambda *x, **k: seen.append(arrays(*x, **k)) or seen[-1]
    out = {"metric": "search_by_sim3 and search_by_sim3_many, one launch each (k_sim3_search)", "rounds": a.rounds}
    if a.feats:
        out["single"] = run_single(a, seen)
    if a.cands:
        out["many"] = run_many(a, seen)
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
