"""What k_local_search buys: Tracking.search_local_points (Frame.is_in_frustum over the local map, then
ORBMatcher.search_by_projection_f_p) from one launch.

Single call: the loop of Tracking.py:439-468 with the reference's per-point frustum test (frame.is_in_frustum_one, the
reference's expressions on one-element arrays) and the existing search_by_projection_f_p, which is what the tree
before this entry offers, against ORBMatcher.search_local_points, on a tests/matcher_world world: a frame of --feats
features (KITTI-size image, 64 x 48 grid) and a local map of P points, P in --points, about 0.7 of the frame's
features re-observing map points; th = 1, nnratio = 0.8, the limit 0.5, a tenth of the points with observations, a
twentieth of the frame's slots pre-filled.

Many: search_local_points_many over --frames frames (copies of the frame, each with slots of its own and a pose moved a
little, all searching the same local map) against the loop of public single calls.

The search assigns into the frame and writes on the map points, so every sample runs on a fresh build of the same
world.  Beside each new call: its kernel time (orbfe_local_search_last_ms), the time inside the entry (staging, launch,
download), the packing before it, the host frustum half (is_in_frustum_many) and the replay after it, the share of
items that came back marked, and the items redone alone.  Every measurement is taken --rounds times in this process,
the variants alternating inside a round; the JSON holds every sample.  --new-only runs the new calls alone (the shape
to put under a kernel trace).

  python tools/bench_local_search.py [--rounds 5] [--points 500 2000 8000] [--feats 2000] [--frames 8] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

TH, LIMIT, NNRATIO = 1, 0.5, 0.8


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4),
            "samples": [round(x, 4) for x in xs]}


def world(points, feats, seed):
    """Arrays of a two-keyframe world of `points` map points; keyframe 1's first `feats` features (its
    re-observations come first) and its pose make the frame."""
    import fuse_cases as FC
    import matcher_world as MW
    rng = np.random.Generator(np.random.PCG64(seed))
    n = max(points, feats)
    z = MW.make_world(rng, n_kf=2, n=n, n_mp=points)
    for k in ("x", "y", "octave", "angle", "desc", "uR", "word"):
        z["kf1_" + k] = z["kf1_" + k][:feats]
    z["ls_obs"] = np.where(rng.random(points) < 0.1, 1, 0).astype(np.int32)
    pre = np.full(feats, -1, np.int32)
    for i in rng.choice(feats, feats // 20, replace=False).tolist():
        pre[i] = int(rng.integers(points))
    z["pre"] = pre
    z["shift"] = rng.normal(0, 0.01, (64, 3)).astype(np.float32)
    return FC.Z(z)


def jobs(z, n):
    """n (frame, local map) on a fresh build; frame k's pose is moved by the k-th seeded shift."""
    import local_search_cases as LC
    import matcher_world as MW
    from pyorbslam_amd import frame as PF

    class Frame(LC.Frame):
        is_in_frustum = PF.is_in_frustum_one

    w = MW.World()
    for i in range(len(z["mp_desc"])):
        p = LC.MapPoint(w, i, z["mp_pos"][i], z["mp_desc"][i], z["mp_normal"][i], z["mp_min"][i], z["mp_max"][i],
                        bool(z["mp_bad"][i]))
        p.nObs = int(z["ls_obs"][i])
        w.mps.append(p)
    a = MW.sub(z, "kf1_")
    out = []
    for k in range(n):
        T = z["kf1_T"].copy()
        if k:
            T[:3, 3] += z["shift"][k]
        F = Frame(w, a, T, mn_id=100 + k)
        F.mvpMapPoints = [w.mps[int(m)] if m >= 0 else None for m in z["pre"]]
        out.append((F, list(w.mps)))
    return out


def state(js, res):
    return [(r, [-1 if p is None else p.mnId for p in j[0].mvpMapPoints],
             [(bool(p.mbTrackInView), p.mnVisible) for p in j[1]]) for r, j in zip(res, js)]


def measure(a, z, n, probe):
    """The loop of n baseline loops, the loop of n public calls (n > 1 only) and the one new call, alternating."""
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher(NNRATIO, True)

    def new(js):
        if n == 1:
            return [m.search_local_points(*js[0], TH, LIMIT)]
        return m.search_local_points_many([j[0] for j in js], [j[1] for j in js], TH, LIMIT)

    def base(js):
        return [m._local_loop(*j, TH, LIMIT) for j in js]
    js = jobs(z, n)
    got = state(js, new(js))
    if not a.new_only:
        js = jobs(z, n)
        assert got == state(js, base(js)), "device path against the loop"
    cols = {k: [] for k in ("base", "loop", "new", "kernel", "entry", "pack", "frustum", "replay", "marked", "redone")}
    for _ in range(a.rounds):
        if not a.new_only:
            js = jobs(z, n)
            t0 = time.perf_counter()
            base(js)
            cols["base"].append((time.perf_counter() - t0) * 1e3)
            if n > 1:
                js = jobs(z, n)
                t0 = time.perf_counter()
                for j in js:
                    m.search_local_points(*j, TH, LIMIT)
                cols["loop"].append((time.perf_counter() - t0) * 1e3)
        js = jobs(z, n)
        probe.reset()
        t0 = time.perf_counter()
        new(js)
        t1 = time.perf_counter()
        cols["new"].append((t1 - t0) * 1e3)
        cols["kernel"].append(matcher.local_search_last_ms())
        cols["entry"].append((probe.entry[1] - probe.entry[0]) * 1e3)
        cols["pack"].append((probe.entry[0] - t0) * 1e3)
        cols["frustum"].append(probe.frustum * 1e3)
        cols["replay"].append((t1 - probe.entry[1] - probe.frustum) * 1e3)
        st = probe.res["status"]
        cols["marked"].append(float(np.count_nonzero(st)) / max(st.size, 1))
        cols["redone"].append(float(probe.ones))
    out = {"searches": n, "items": int(probe.res["status"].size), "in_view": int(probe.res["in_view"].sum()),
           "results": [list(g[0]) for g in got], "new_ms": spread(cols["new"]), "kernel_ms": spread(cols["kernel"]),
           "entry_ms": spread(cols["entry"]), "packing_ms": spread(cols["pack"]),
           "host_frustum_ms": spread(cols["frustum"]), "replay_ms": spread(cols["replay"]),
           "marked_share_of_items": spread(cols["marked"]), "items_redone_alone": spread(cols["redone"])}
    if not a.new_only:
        out["baseline_loop_ms"] = spread(cols["base"])
        out["baseline_median_over_new_median"] = round(out["baseline_loop_ms"]["median"] / out["new_ms"]["median"], 3)
        out["every_new_sample_below_every_baseline_sample"] = max(cols["new"]) < min(cols["base"])
        if n > 1:
            out["loop_of_single_calls_ms"] = spread(cols["loop"])
    return out


class Probe:
    """Time stamps around the entry and inside the host frustum half, the last results, the single redos."""

    def __init__(self):
        from pyorbslam_amd import frame as PF
        from pyorbslam_amd import matcher
        arrays, one, many = matcher.local_search_arrays, matcher.ORBMatcher._fp_one, PF.is_in_frustum_many

        def entry(*x, **k):
            t0 = time.perf_counter()
            self.res = arrays(*x, **k)
            self.entry = (t0, time.perf_counter())
            return self.res

        def frustum(*x):
            t0 = time.perf_counter()
            r = many(*x)
            self.frustum += time.perf_counter() - t0
            return r

        def fp_one(m, *x):
            self.ones += 1
            return one(m, *x)
        matcher.local_search_arrays, matcher.ORBMatcher._fp_one, PF.is_in_frustum_many = entry, fp_one, frustum
        self.reset()

    def reset(self):
        self.entry, self.frustum, self.ones, self.res = (0.0, 0.0), 0.0, 0, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", type=int, nargs="*", default=[500, 2000, 8000])
    ap.add_argument("--feats", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--many-points", type=int, default=2000)
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    probe = Probe()
    out = {"metric": "search_local_points and search_local_points_many, one launch each (k_local_search)",
           "th": TH, "limit": LIMIT, "nnratio": NNRATIO, "features": a.feats, "rounds": a.rounds, "single": {}}
    for P in a.points:
        out["single"][str(P)] = dict(points=P, **measure(a, world(P, a.feats, 17), 1, probe))
        print(f"single {P}: done", file=sys.stderr, flush=True)
    if a.frames:
        out["many"] = dict(points=a.many_points, **measure(a, world(a.many_points, a.feats, 13), a.frames, probe))
        print("many: done", file=sys.stderr, flush=True)
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
