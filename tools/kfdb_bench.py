"""Place-recognition benchmark: KeyFrameDatabase on the device against the reference's algorithm on this host.

Databases are seed-generated at ORBvoc's shape: vectors of about 1 500 words over a 10^6-word vocabulary,
clustered into places so that neighbours share words, and a 1 500-word query.  Per database size it reports
  kernel_ms       k_bow_score alone (orbfe_kfdb_last_ms, HIP events), mean over the timed window
  call_ms         a whole detect_loop_candidates call (query upload, launch, result download, host replay);
                  the call ends in a stream synchronise, so the host clock around it is the latency
  add_us          one KeyFrameDatabase.add (BoW dict -> slot; no device call)
  hbm_share       algorithmic bytes (4 B per stored word + 8 B per hit + the query) / kernel time / HBM peak
  kernel_ms_nq    kernel time with the query cut to 1 and 32 words: every stored word is still streamed but the
                  binary search is 1 or 6 steps deep instead of 11, which separates the streaming cost from the
                  search cost and says which of the two bounds the kernel
and, at 1 024 and 4 096 vectors, baseline_ms: the pure-Python inverted-file walk plus scoring of
tests/kfdb_oracle.py (the reference's algorithm) on this host, in the same run.

Usage:  python tools/kfdb_bench.py [--out profiles/kfdb] [--sizes 1024,4096,16384]
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

N_WORDS = 1_000_000
VEC_WORDS = 1500
POOL = 6000            # words a place draws from
PER_PLACE = 64         # keyframes per place
HBM_PEAK = 8.0e12      # B/s, MI355X HBM3E specification
DICT_LIMIT = 4096      # above this the stand-ins carry array-backed vectors (24 M dict entries otherwise)


class ArrayBow:
    """A BoW vector kept as two arrays with the mapping methods KeyFrameDatabase.add reads."""

    def __init__(self, word, weight):
        self.word, self.weight = word, weight

    def __len__(self):
        return len(self.word)

    def keys(self):
        return self.word

    def values(self):
        return self.weight


class KF:
    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = bow
        self.mnLoopQuery = self.mnLoopWords = self.mnRelocQuery = self.mnRelocWords = 0
        self.mRelocScore = 0.0
        self.connected = set()
        self.covis = []

    def get_connected_key_frames(self):
        return set(self.connected)

    def get_best_covisibility_key_frames(self, n):
        return self.covis[:n]


def vector(r, pool):
    own = r.choice(pool, int(VEC_WORDS * 0.8), replace=False)
    rest = r.integers(0, N_WORDS, VEC_WORDS - len(own))
    w = np.unique(np.concatenate([own, rest])).astype(np.int32)
    v = r.random(len(w)) + 0.05
    return w, v / v.sum()


def make_world(n, seed=1):
    r = np.random.default_rng(seed)
    n_places = max(1, n // PER_PLACE)
    pools = [r.choice(N_WORDS, POOL, replace=False) for _ in range(n_places)]
    kfs = []
    for i in range(n):
        w, v = vector(r, pools[i * n_places // n])
        bow = dict(zip(w.tolist(), v.tolist())) if n <= DICT_LIMIT else ArrayBow(w, v)
        kfs.append(KF(i + 1, bow))
    for i, kf in enumerate(kfs):
        kf.covis = [kfs[j] for j in range(max(0, i - 6), min(n, i + 7)) if j != i]
    queries = []
    for k in range(8):  # queries revisit places spread over the map; their neighbours are not in the database
        w, v = vector(r, pools[(k * 37 + 3) % n_places])
        queries.append((w, v))
    return kfs, queries


def query_kf(qid, wv, as_dict):
    w, v = wv
    return KF(qid, dict(zip(w.tolist(), v.tolist())) if as_dict else ArrayBow(w, v))


def bench_size(n, window_s):
    import torch
    from pyorbslam_amd.kfdb import KeyFrameDatabase
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    t0 = time.perf_counter()
    kfs, queries = make_world(n)
    gen_s = time.perf_counter() - t0
    as_dict = n <= DICT_LIMIT
    db = KeyFrameDatabase(TemplatedVocabulary())
    t0 = time.perf_counter()
    for kf in kfs:
        db.add(kf)
    add_us = (time.perf_counter() - t0) / n * 1e6
    stored = db._db.stats()["live_words"]
    qid = 10 * n
    for k in range(3):  # warm-up: first launch loads the code object, first query uploads the database
        qid += 1
        db.detect_loop_candidates(query_kf(qid, queries[k % len(queries)], as_dict), 0.0)
    torch.cuda.synchronize()
    call, kern, hits, cands = [], [], 0, 0
    t_end = time.perf_counter() + window_s
    k = 0
    while time.perf_counter() < t_end or k < 20:
        qid += 1
        q = query_kf(qid, queries[k % len(queries)], as_dict)
        t0 = time.perf_counter()
        got = db.detect_loop_candidates(q, 0.0)
        call.append(time.perf_counter() - t0)
        kern.append(db.last_kernel_ms())
        cands += len(got)
        k += 1
    # hits of the eight distinct queries, for the algorithmic bytes
    per_q_hits = []
    for wv in queries:
        common, _, _ = db._db.query_arrays(*wv)
        per_q_hits.append(int(common.sum()))
    hits = float(np.mean(per_q_hits))
    kernel_ms = float(np.mean(kern))
    algo_bytes = 4.0 * stored + 8.0 * hits + 12.0 * VEC_WORDS
    short = {}
    for nq in (1, 32):
        w, v = queries[0]
        ms = []
        for _ in range(30):
            db._db.query_arrays(w[:nq], v[:nq])
            ms.append(db.last_kernel_ms())
        short[str(nq)] = float(np.mean(ms[5:]))
    res = dict(n_vectors=n, stored_words=int(stored), query_words=int(len(queries[0][0])), queries_timed=k,
               window_s=float(sum(call)), kernel_ms=kernel_ms, kernel_ms_min=float(np.min(kern)),
               call_ms=float(np.mean(call) * 1e3), call_ms_median=float(np.median(call) * 1e3), add_us=add_us,
               add_from="dict" if as_dict else "arrays", hits_per_query=hits, candidates_per_query=cands / k,
               algo_bytes=algo_bytes, hbm_share=algo_bytes / (kernel_ms * 1e-3) / HBM_PEAK, kernel_ms_nq=short,
               world_gen_s=gen_s)
    return res, kfs, queries


def baseline(kfs, queries, n_queries=3):
    """The reference's algorithm in Python on this host: inverted file walk, word gate, l1 scoring."""
    import kfdb_oracle as KO
    db = KO.OracleKeyFrameDatabase()
    t0 = time.perf_counter()
    for kf in kfs:
        db.add(kf)
    add_us = (time.perf_counter() - t0) / len(kfs) * 1e6
    ts = []
    for k in range(n_queries):
        q = query_kf(5_000_000 + k, queries[k], True)
        t0 = time.perf_counter()
        db.detect_loop_candidates(q, 0.0)
        ts.append(time.perf_counter() - t0)
    return dict(baseline_ms=float(np.mean(ts) * 1e3), baseline_ms_min=float(np.min(ts) * 1e3),
                baseline_add_us=add_us, baseline_queries=n_queries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kfdb"))
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--window", type=float, default=1.5, help="timed window per size, seconds")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "kfdb_bench needs a GPU: there is no CPU path to time"
    from pyorbslam_amd import _lib
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    rows = []
    for n in (int(x) for x in args.sizes.split(",")):
        res, kfs, queries = bench_size(n, args.window)
        if n <= DICT_LIMIT:
            res.update(baseline(kfs, queries))
            res["speedup_call"] = res["baseline_ms"] / res["call_ms"]
        rows.append(res)
        print(json.dumps(res), flush=True)
        del kfs
    doc = dict(build_id=_lib.build_id(), device=torch.cuda.get_device_name(0), gpus=1,
               note="measured on one MI355X; baseline_ms is tests/kfdb_oracle.py on the same host in the same run",
               hbm_peak_bytes_per_s=HBM_PEAK, sizes=rows)
    (out / "kfdb_bench.json").write_text(json.dumps(doc, indent=1) + "\n")
    print("wrote", out / "kfdb_bench.json")


if __name__ == "__main__":
    main()
