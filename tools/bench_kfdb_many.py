"""Many-query place recognition against a loop of single queries, on the worlds of tools/kfdb_bench.py.

Per database size (1 024 / 4 096 / 16 384 vectors of about 1 500 words, 1 500-word queries) and per Q (1, 16, 64):
  many_us_per_query   host clock around BowDatabase.query_many_arrays(gate_ratio=0.8) (upload, k_bow_score_many,
                      k_bow_gate, the survivors' download; the call ends in a stream synchronise), over Q
  loop_us_per_query   the same Q queries through BowDatabase.query_arrays one after the other (one launch, one
                      synchronise and three dense arrays per query; no gate: that would be host work on top)
  many_kernel_ms      both kernels of the many call (orbfe_kfdb_many_last_ms, HIP events)
  loop_kernel_ms      Q single launches: the sum of orbfe_kfdb_last_ms over the loop
  bytes_down          bytes copied to the host per query by either path
Every figure is the median of --repeats timed repeats (the two paths alternate inside one process, after a warm-up
of both), with the smallest and the largest repeat beside it: a difference counts when the two ranges do not
overlap.

Usage:  python tools/bench_kfdb_many.py [--out profiles/kfdb_many] [--sizes 1024,4096,16384] [--queries 1,16,64]
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
sys.path.insert(0, str(ROOT / "tools"))

import kfdb_bench as KB  # noqa: E402


def make_world(n, n_queries, seed=1):
    """kfdb_bench.make_world's vectors (places of PER_PLACE keyframes drawing from pools of POOL words) as arrays,
    and n_queries queries that revisit places spread over the map."""
    r = np.random.default_rng(seed)
    n_places = max(1, n // KB.PER_PLACE)
    pools = [r.choice(KB.N_WORDS, KB.POOL, replace=False) for _ in range(n_places)]
    stored = [KB.vector(r, pools[i * n_places // n]) for i in range(n)]
    queries = [KB.vector(r, pools[(k * 37 + 3) % n_places]) for k in range(n_queries)]
    return stored, queries


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def bench_size(n, q_counts, repeats):
    import torch
    from pyorbslam_amd import kfdb
    stored, queries = make_world(n, max(q_counts))
    db = kfdb.BowDatabase(n, n * KB.VEC_WORDS)
    for w, v in stored:
        db.add_arrays(w, v)
    cap = min(n, kfdb.HIT_CAP_FIRST)
    rows = []
    for nq in q_counts:
        words, weights = [q[0] for q in queries[:nq]], [q[1] for q in queries[:nq]]

        inner = max(1, 64 // nq)  # every repeat asks 64 queries or more, whatever Q

        def many():
            kern = 0.0
            t0 = time.perf_counter()
            for _ in range(inner):
                recs = db.query_many_arrays(words, weights, gate_ratio=0.8, hit_cap=cap)
                kern += db.last_many_kernel_ms()
            return (time.perf_counter() - t0) / (inner * nq) * 1e6, kern / inner, recs

        def loop():
            kern = 0.0
            t0 = time.perf_counter()
            for _ in range(inner):
                for w, v in zip(words, weights):
                    db.query_arrays(w, v)
                    kern += db.last_kernel_ms()
            return (time.perf_counter() - t0) / (inner * nq) * 1e6, kern / inner

        for _ in range(2):  # warm-up: code objects, the database upload, the scratch and pinned buffers
            many()
            loop()
        torch.cuda.synchronize()
        m_us, m_ms, l_us, l_ms = [], [], [], []
        for _ in range(repeats):
            us, ms, recs = many()
            m_us.append(us)
            m_ms.append(ms)
            us, ms = loop()
            l_us.append(us)
            l_ms.append(ms)
        assert all(r["n_hits"] <= cap for r in recs), "hit_cap overflowed: the timed call is not the whole answer"
        row = dict(n_vectors=n, stored_words=db.stats()["live_words"], n_query=nq, repeats=repeats, hit_cap=cap,
                   many_us_per_query=spread(m_us), loop_us_per_query=spread(l_us),
                   many_kernel_ms=spread(m_ms), loop_kernel_ms=spread(l_ms),
                   speedup_wall=float(np.median(l_us) / np.median(m_us)),
                   kernel_ratio_many_over_loop=float(np.median(m_ms) / np.median(l_ms)),
                   wall_ranges_disjoint=bool(np.max(m_us) < np.min(l_us)),
                   bytes_down_many=12 + 20 * cap, bytes_down_loop=16 * n,
                   hits_per_query=float(np.mean([r["n_hits"] for r in recs])))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kfdb_many"))
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--queries", default="1,16,64")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tag", default="", help="suffix of the output files (A/B builds under ORBFE_LIB)")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least five repeats per figure")
    import torch
    assert torch.cuda.is_available(), "bench_kfdb_many needs a GPU: there is no CPU path to time"
    from pyorbslam_amd import _lib
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    rows = []
    for n in (int(x) for x in args.sizes.split(",")):
        rows += bench_size(n, [int(x) for x in args.queries.split(",")], args.repeats)
    name = "bench_kfdb_many" + (f"_{args.tag}" if args.tag else "")
    (out / f"{name}.txt").write_text("".join(json.dumps(r) + "\n" for r in rows))
    doc = dict(build_id=_lib.build_id(), lib=str(_lib.LIB_PATH.name), device=torch.cuda.get_device_name(0), gpus=1,
               note="measured on one MI355X; both paths in one process, alternating", rows=rows)
    (out / f"{name}.json").write_text(json.dumps(doc, indent=1) + "\n")
    print("wrote", out / f"{name}.json")


if __name__ == "__main__":
    main()
