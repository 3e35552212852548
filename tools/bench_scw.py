"""What k_scw_search buys: loop closing's two Sim3 projection searches from one launch each.

Shape 1, LoopClosing.search_and_fuse: ORBMatcher.fuse_kf_scw_mp once per keyframe of the corrected poses with the
loop's map points and th = 4, the replace loop after each.  The loop of N single calls plus the replace (one
k_hamming_search launch, a Python projection and a Python replay each; still in the tree, so it is the baseline)
against one fuse_kf_scw_mp_many(..., after=replace), N in --kfs, on a tests/matcher_world world of `--feats` features
per keyframe; with --clones a share of the keyframes' slots holds a clone of the point they re-observe
(tests/fuse_cases.clone_world), so that points get replaced and the survivors' changed descriptors send items of
later keyframes through the single-item path.

Shape 2, LoopClosing.compute_sim3: search_by_projection_ckf_scw_mp of P map points into one keyframe of P features
with th = 10, P in --ckf-points; vpMatched is pre-filled at every third feature whose slot holds a map point (the
JSON has the count).  The host body (_ckf_host, the former body of the public method) against the public method.

Fusing changes the map, so every sample runs on a fresh build of the same world.  Beside each new call: its kernel
time (orbfe_scw_search_last_ms), the time of packing keyframes and points into arrays on a fresh build, and the share
of items that came back marginal.  Every measurement is taken --rounds times, the variants alternating inside a
round; the JSON holds every sample.  --many-only runs the new calls alone (the shape to put under a kernel trace).

  python tools/bench_scw.py [--rounds 3] [--kfs 1 10 30] [--feats 2000] [--ckf-points 2000 8000] [--clones] [--out FILE]
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

TH_FUSE, TH_CKF = 4.0, 10.0
SCALES = (1.0, 1.1, 0.9)


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
    _lib.call("orbfe_scw_search_last_ms", C.byref(ms))
    return ms.value


def fuse_shape(w, n):
    import matcher_world as MW
    import scw_cases as SC
    kfs = w.kfs[1:1 + n]
    pts = SC.loop_points(w)
    return kfs, [MW.sim3(kf.Tcw, SCALES[j % 3]) for j, kf in enumerate(kfs)], pts, SC.replacer(pts)


def encode(res):
    return [(int(n), [-1 if p is None else p.mnId for p in rep]) for n, rep in res]


def run_fuse(a, seen):
    import fuse_cases as FC
    import matcher_world as MW
    import scw_cases as SC
    from pyorbslam_amd import matcher
    n_max = max(a.kfs)
    if a.clones:
        z = FC.Z(FC.clone_world(13, n_kf=n_max + 1, n=a.feats, n_mp=int(a.feats * 0.7)))
    else:
        z = FC.Z(MW.make_world(np.random.Generator(np.random.PCG64(13)), n_kf=n_max + 1, n=a.feats,
                               n_mp=int(a.feats * 0.7)))
    m = matcher.ORBMatcher()
    loop_of_singles = SC.loop_fuse(m.fuse_kf_scw_mp)
    out = {"features": a.feats, "world": "clone_world" if a.clones else "make_world"}
    for n in a.kfs:
        # warm-up of both, and the equality of what they return
        w = fresh(z)
        kfs, S, pts, rep = fuse_shape(w, n)
        got = encode(m.fuse_kf_scw_mp_many(kfs, S, pts, TH_FUSE, rep))
        n_replace = sum(1 for e in w.log if e[0] == MW.EV_REPLACE)
        if not a.many_only:
            w = fresh(z)
            kfs, S, pts, rep = fuse_shape(w, n)
            assert got == encode(loop_of_singles(kfs, S, pts, TH_FUSE, rep))
        loop, many, pack, kern, marg = [], [], [], [], []
        for _ in range(a.rounds):
            if not a.many_only:
                w = fresh(z)
                kfs, S, pts, rep = fuse_shape(w, n)
                t0 = time.perf_counter()
                loop_of_singles(kfs, S, pts, TH_FUSE, rep)
                loop.append((time.perf_counter() - t0) * 1e3)
            w = fresh(z)
            kfs, S, pts, rep = fuse_shape(w, n)
            del seen[:]
            t0 = time.perf_counter()
            m.fuse_kf_scw_mp_many(kfs, S, pts, TH_FUSE, rep)
            many.append((time.perf_counter() - t0) * 1e3)
            kern.append(last_ms())
            st = seen[0]["status"]
            marg.append(float(np.count_nonzero(st)) / max(st.size, 1))
            w = fresh(z)
            kfs, S, pts, rep = fuse_shape(w, n)
            t0 = time.perf_counter()
            for kf, Scw in zip(kfs, S):
                m._scw_frame(kf, Scw, m._sim3_to_pose)
            for p in pts:
                if not p.is_bad():
                    matcher._fuse_point(p)
            pack.append((time.perf_counter() - t0) * 1e3)
        out[str(n)] = {"replace_events": n_replace, "keyframes": len(kfs), "points": len(pts),
                       "items": int(seen[0]["status"].size), "many_ms": spread(many), "many_packing_ms": spread(pack),
                       "many_kernel_ms": spread(kern), "marginal_share_of_items": spread(marg),
                       "fused": [g[0] for g in got]}
        if not a.many_only:
            out[str(n)]["loop_ms"] = spread(loop)
            out[str(n)]["every_new_sample_below_every_baseline_sample"] = max(many) < min(loop)
        print(f"search_and_fuse {n}: done", file=sys.stderr, flush=True)
    return out


def ckf_shape(w, z):
    import matcher_world as MW
    kf = w.kfs[1]
    vm = [w.mps[int(i)] if i >= 0 and j % 3 == 0 else None for j, i in enumerate(z["kfmp1"])]
    return kf, MW.sim3(kf.Tcw, 1.1), list(w.mps), vm


def run_ckf(a, seen):
    import fuse_cases as FC
    import matcher_world as MW
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    enc = lambda r: (int(r[0]), [-1 if p is None else p.mnId for p in r[1]])  # noqa: E731
    out = {}
    for P in a.ckf_points:
        z = FC.Z(MW.make_world(np.random.Generator(np.random.PCG64(17)), n_kf=2, n=P, n_mp=P))
        got = enc(m.search_by_projection_ckf_scw_mp(*ckf_shape(fresh(z), z), TH_CKF))
        if not a.many_only:
            assert got == enc(m._ckf_host(*ckf_shape(fresh(z), z), TH_CKF))
        host, dev, pack, kern, marg = [], [], [], [], []
        for _ in range(a.rounds):
            if not a.many_only:
                args = ckf_shape(fresh(z), z)
                t0 = time.perf_counter()
                m._ckf_host(*args, TH_CKF)
                host.append((time.perf_counter() - t0) * 1e3)
            args = ckf_shape(fresh(z), z)
            del seen[:]
            t0 = time.perf_counter()
            m.search_by_projection_ckf_scw_mp(*args, TH_CKF)
            dev.append((time.perf_counter() - t0) * 1e3)
            kern.append(last_ms())
            st = seen[0]["status"]
            marg.append(float(np.count_nonzero(st)) / max(st.size, 1))
            kf, Scw, pts, vm = ckf_shape(fresh(z), z)
            t0 = time.perf_counter()
            m._scw_frame(kf, Scw, m._ckf_pose)
            found = set(vm) - {None}
            for p in pts:
                if not (p.is_bad() or p in found):
                    matcher._fuse_point(p)
            pack.append((time.perf_counter() - t0) * 1e3)
        out[str(P)] = {"points": P, "features": P, "prefilled": sum(v is not None for v in ckf_shape(fresh(z), z)[3]),
                       "items": int(seen[0]["status"].size), "matches": got[0], "device_ms": spread(dev),
                       "device_packing_ms": spread(pack), "device_kernel_ms": spread(kern),
                       "marginal_share_of_items": spread(marg)}
        if not a.many_only:
            out[str(P)]["host_ms"] = spread(host)
            out[str(P)]["every_new_sample_below_every_baseline_sample"] = max(dev) < min(host)
        print(f"ckf {P}: done", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kfs", type=int, nargs="*", default=[1, 10, 30])
    ap.add_argument("--feats", type=int, default=2000)
    ap.add_argument("--ckf-points", type=int, nargs="*", default=[2000, 8000])
    ap.add_argument("--many-only", action="store_true")
    ap.add_argument("--clones", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pyorbslam_amd import matcher
    seen = []
    arrays = matcher.scw_search_arrays
    matcher.scw_search_arrays = lambda *x, **k: seen.append(arrays(*x, **k)) or seen[-1]
    out = {"metric": "fuse_kf_scw_mp over many keyframes and search_by_projection_ckf_scw_mp, one launch each "
                     "(k_scw_search)", "rounds": a.rounds}
    if a.kfs:
        out["search_and_fuse"] = run_fuse(a, seen)
    if a.ckf_points:
        out["ckf"] = run_ckf(a, seen)
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
