"""What k_fkf_search buys: Tracking.relocalization's projection search, ORBMatcher.search_by_projection_f_kf_f, from
one launch.

Single call: the host body (_fkf_host, the former body of the public method, so it is the baseline) against the public
method on a tests/matcher_world world: a keyframe of P features whose slots hold about 0.9 P map points, searched in a
frame of P features that re-observes them, P in --feats; th = 10, ORBdist = 100, a quarter of the frame's slots
pre-filled, a tenth of the keyframe's points in sAlreadyFound.

Many: search_by_projection_f_kf_f_many over --frames frames of --many-feats features (copies of the frame, each with
slots of its own and a pose moved a little) against the loop of public single calls.

The search assigns into the frame, so every sample runs on a fresh build of the same world.  Beside each new call: its
kernel time (orbfe_fkf_search_last_ms), the share of items that came back marked, and the items redone alone.  Every
measurement is taken --rounds times in this process, the variants alternating inside a round; the JSON holds every
sample.  --new-only runs the new calls alone (the shape to put under a kernel trace).

  python tools/bench_fkf.py [--rounds 5] [--feats 500 2000 8000] [--frames 8] [--many-feats 2000] [--out FILE]
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

TH, ORB_DIST = 10.0, 100


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4),
            "samples": [round(x, 4) for x in xs]}


def last_ms():
    from pyorbslam_amd import _lib
    ms = C.c_float()
    _lib.call("orbfe_fkf_search_last_ms", C.byref(ms))
    return ms.value


def world(feats, seed):
    """Arrays of a two-keyframe world; keyframe 1's features and pose make the frame."""
    import fuse_cases as FC
    import matcher_world as MW
    rng = np.random.Generator(np.random.PCG64(seed))
    z = MW.make_world(rng, n_kf=2, n=feats, n_mp=feats)
    held = np.unique(z["kfmp0"][z["kfmp0"] >= 0])
    z["found"] = rng.choice(held, max(1, len(held) // 10), replace=False).astype(np.int32)
    pre = np.full(feats, -1, np.int32)
    for i in rng.choice(feats, feats // 4, replace=False).tolist():
        pre[i] = z["kfmp1"][i] if z["kfmp1"][i] >= 0 else int(rng.integers(feats))
    z["pre"] = pre
    z["shift"] = rng.normal(0, 0.01, (64, 3)).astype(np.float32)
    return FC.Z(z)


def jobs(z, n):
    """n (frame, keyframe 0, sAlreadyFound) on a fresh build; frame k's pose is moved by the k-th seeded shift."""
    import fkf_cases as KC
    import matcher_world as MW
    w = MW.build(z)
    a = MW.sub(z, "kf1_")
    found = {w.mps[int(m)] for m in z["found"]}
    out = []
    for k in range(n):
        T = z["kf1_T"].copy()
        if k:
            T[:3, 3] += z["shift"][k]
        F = KC.Frame(w, a, T)
        F.mvpMapPoints = [w.mps[int(m)] if m >= 0 else None for m in z["pre"]]
        out.append((F, w.kfs[0], found))
    return out


def state(js, ns):
    return [(int(n), [-1 if p is None else p.mnId for p in j[0].mvpMapPoints]) for n, j in zip(ns, js)]


def measure(a, z, n, seen, ones):
    """The loop of n host bodies, the loop of n public calls (n > 1 only) and the one new call, alternating."""
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()

    def new(js):
        if n == 1:
            return [m.search_by_projection_f_kf_f(*js[0], TH, ORB_DIST)]
        return m.search_by_projection_f_kf_f_many(*[[j[c] for j in js] for c in range(3)], TH, ORB_DIST)
    js = jobs(z, n)
    got = state(js, new(js))
    if not a.new_only:
        js = jobs(z, n)
        assert got == state(js, [m._fkf_host(*j, TH, ORB_DIST) for j in js]), "device path against the host body"
    host, loop, dev, kern, marg, redo = [], [], [], [], [], []
    for _ in range(a.rounds):
        if not a.new_only:
            js = jobs(z, n)
            t0 = time.perf_counter()
            for j in js:
                m._fkf_host(*j, TH, ORB_DIST)
            host.append((time.perf_counter() - t0) * 1e3)
            if n > 1:
                js = jobs(z, n)
                t0 = time.perf_counter()
                for j in js:
                    m.search_by_projection_f_kf_f(*j, TH, ORB_DIST)
                loop.append((time.perf_counter() - t0) * 1e3)
        js = jobs(z, n)
        del seen[:], ones[:]
        t0 = time.perf_counter()
        new(js)
        dev.append((time.perf_counter() - t0) * 1e3)
        kern.append(last_ms())
        st = seen[0]["status"]
        marg.append(float(np.count_nonzero(st)) / max(st.size, 1))
        redo.append(float(len(ones)))
    out = {"searches": n, "items": int(seen[0]["status"].size), "matches": [g[0] for g in got],
           "device_ms": spread(dev), "device_kernel_ms": spread(kern), "marked_share_of_items": spread(marg),
           "items_redone_alone": spread(redo)}
    if not a.new_only:
        out["host_body_ms"] = spread(host)
        out["device_median_below_host_median"] = out["device_ms"]["median"] < out["host_body_ms"]["median"]
        out["every_new_sample_below_every_baseline_sample"] = max(dev) < min(host)
        if n > 1:
            out["loop_of_single_calls_ms"] = spread(loop)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--feats", type=int, nargs="*", default=[500, 2000, 8000])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--many-feats", type=int, default=2000)
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pyorbslam_amd import matcher
    seen, ones = [], []
    arrays, one = matcher.fkf_search_arrays, matcher.ORBMatcher._fkf_one
    matcher.fkf_search_arrays = lambda *x, **k: seen.append(arrays(*x, **k)) or seen[-1]
    matcher.ORBMatcher._fkf_one = lambda self, *x: ones.append(1) or one(self, *x)
    out = {"metric": "search_by_projection_f_kf_f and search_by_projection_f_kf_f_many, one launch each (k_fkf_search)",
           "th": TH, "orb_dist": ORB_DIST, "rounds": a.rounds, "single": {}}
    for P in a.feats:
        out["single"][str(P)] = dict(features=P, **measure(a, world(P, 17), 1, seen, ones))
        print(f"single {P}: done", file=sys.stderr, flush=True)
    if a.frames:
        out["many"] = dict(features=a.many_feats, **measure(a, world(a.many_feats, 13), a.frames, seen, ones))
        print("many: done", file=sys.stderr, flush=True)
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
