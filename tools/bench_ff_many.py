"""What k_ff_search buys: ORBMatcher.search_by_projection_f_f for many (current frame, last frame) pairs from one launch.

search_by_projection_f_f_many against the loop of the existing single calls, on the worlds of the golden's generator
(tests/golden/gen_golden_ff_many.py) at --feats features a frame: 1 and --pairs pairs, in a float64 world (where the
single call takes its native selection, every compared operand being a double) and in a float32 world (where it takes
its per-item Python loop).  th alternates 7 / 15 and the motion mode cycles over the pairs, as in the golden.

The search assigns into the current frames, so every sample runs on a fresh build of the same world.  Beside the new
call: its kernel time (orbfe_ff_search_last_ms), the time inside the entry (staging, launch, download), the packing
before it and the replay after it, the share of items that came back marked, and the items redone alone.  Every
measurement is taken --rounds times in this process, the variants alternating inside a round; the JSON holds every
sample.

  python tools/bench_ff_many.py [--rounds 5] [--feats 2000] [--pairs 8] [--out FILE]
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
sys.path.insert(0, str(ROOT / "tests" / "golden"))


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4),
            "samples": [round(x, 4) for x in xs]}


def world(n_pairs, feats, dtype, seed):
    import gen_golden_ff_many as G
    rng = np.random.Generator(np.random.PCG64(seed))
    z = G.Npz()
    for k in range(n_pairs):
        z.update({f"p{k}_{key}": v for key, v in G.pair(rng, k, feats, dtype).items()})
    return z


def jobs(z, n):
    import ff_cases as FC
    pairs = [FC.load_pair(z, k) for k in range(n)]
    return [(p[0], p[1], p[4]) for p in pairs]


def state(js, res):
    return [(r, [id(m) if m is not None else 0 for m in j[0].mvpMapPoints].count(0)) for r, j in zip(res, js)]


class Probe:
    """Time stamps around the entry, the last results, the single redos."""

    def __init__(self):
        from pyorbslam_amd import matcher
        arrays, one = matcher.ff_search_arrays, matcher.ORBMatcher._ff_one

        def entry(*x, **k):
            t0 = time.perf_counter()
            self.res = arrays(*x, **k)
            self.entry = (t0, time.perf_counter())
            return self.res

        def ff_one(m, *x):
            self.ones += 1
            return one(m, *x)
        matcher.ff_search_arrays, matcher.ORBMatcher._ff_one = entry, ff_one
        self.reset()

    def reset(self):
        self.entry, self.ones, self.res = (0.0, 0.0), 0, None


def measure(a, z, n, probe):
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher(0.8, True)

    def new(js):
        return m.search_by_projection_f_f_many([j[0] for j in js], [j[1] for j in js], [j[2] for j in js])

    def loop(js):
        return [m.search_by_projection_f_f(*j) for j in js]
    js = jobs(z, n)
    got = state(js, new(js))
    js = jobs(z, n)
    assert got == state(js, loop(js)), "the many call against the loop of single calls"
    cols = {k: [] for k in ("loop", "new", "kernel", "entry", "pack", "replay", "marked", "redone")}
    for _ in range(a.rounds):
        js = jobs(z, n)
        t0 = time.perf_counter()
        loop(js)
        cols["loop"].append((time.perf_counter() - t0) * 1e3)
        js = jobs(z, n)
        probe.reset()
        t0 = time.perf_counter()
        new(js)
        t1 = time.perf_counter()
        cols["new"].append((t1 - t0) * 1e3)
        cols["kernel"].append(matcher.ff_search_last_ms())
        cols["entry"].append((probe.entry[1] - probe.entry[0]) * 1e3)
        cols["pack"].append((probe.entry[0] - t0) * 1e3)
        cols["replay"].append((t1 - probe.entry[1]) * 1e3)
        st = probe.res["status"]
        cols["marked"].append(float(np.count_nonzero(st)) / max(st.size, 1))
        cols["redone"].append(float(probe.ones))
    out = {"pairs": n, "items": int(probe.res["status"].size), "matches": [g[0] for g in got],
           "new_ms": spread(cols["new"]), "loop_of_single_calls_ms": spread(cols["loop"]),
           "kernel_ms": spread(cols["kernel"]), "entry_ms": spread(cols["entry"]), "packing_ms": spread(cols["pack"]),
           "replay_ms": spread(cols["replay"]), "marked_share_of_items": spread(cols["marked"]),
           "items_redone_alone": spread(cols["redone"])}
    out["loop_median_over_new_median"] = round(out["loop_of_single_calls_ms"]["median"] / out["new_ms"]["median"], 3)
    out["every_new_sample_below_every_loop_sample"] = max(cols["new"]) < min(cols["loop"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--feats", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    probe = Probe()
    out = {"metric": "search_by_projection_f_f_many, one launch (k_ff_search), against the loop of single calls",
           "features": a.feats, "rounds": a.rounds, "worlds": {}}
    for name, dtype in (("float64", np.float64), ("float32", np.float32)):
        z = world(a.pairs, a.feats, dtype, 23)
        out["worlds"][name] = {str(n): measure(a, z, n, probe) for n in sorted({1, a.pairs})}
        print(f"{name}: done", file=sys.stderr, flush=True)
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
