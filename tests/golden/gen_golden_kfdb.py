"""Generate place-recognition goldens from the REFERENCE KeyFrameDatabase (build container only).

Imports the reference's KeyFrameDatabase and pyDBoW.ScoringObject read-only from the directory given on the
command line and runs them on stand-in keyframes (tests/kfdb_oracle.py: mnId, mBowVec, the query attributes as
KeyFrame.__init__ sets them, a connected set and an ordered covisibility list of up to 15).  Records per case in
tests/golden/kfdb_<case>.npz the inputs, the operation sequence and, after every query, the returned keyframes
plus every keyframe's six attributes (a presence flag for mLoopScore) and which query keyframe last set each
score (for the tests' error bound).

Every recorded query is also run through the canonical-order oracle (kfdb_oracle.OracleKeyFrameDatabase): the
id lists and integer attributes must be identical, or the generator stops.  Nothing here runs on the GPU box.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_kfdb.py <reference root>
"""
from __future__ import annotations

import sys
from collections import OrderedDict
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[2]
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, sys.argv[1])

import kfdb_oracle as KO  # noqa: E402
from KeyFrameDatabase import KeyFrameDatabase  # noqa: E402
from pyDBoW.ScoringObject import GeneralScoring  # noqa: E402

N_WORDS = 400
N_PLACES = 6
CASES = [("w0", 101), ("w1", 202), ("w2", 303)]


class RecordingVoc:
    """GeneralScoring.l1_score, remembering which query vector scored which keyframe's."""

    def __init__(self):
        self.pairs = []

    def score(self, v1, v2):
        self.pairs.append((id(v1), id(v2)))
        return GeneralScoring.l1_score(v1, v2)


def make_world(seed):
    """About 60 keyframes in places that share word pools, plus 4 query-only stand-ins."""
    r = np.random.default_rng(seed)
    pools = [r.choice(N_WORDS, 150, replace=False) for _ in range(N_PLACES)]
    n_db = 60
    place = np.sort(r.integers(0, N_PLACES, n_db))
    place = np.concatenate([place, r.integers(0, N_PLACES, 4)])  # the last four only query
    ids = list(range(1, n_db + 1)) + [0, 17, 900, 901]            # mnId 0, and one that repeats keyframe 17's
    bows = []
    for p in place:
        k = int(r.integers(40, 121))
        n_own = int(k * 0.85)
        own = r.choice(pools[p], n_own, replace=False)
        rest = r.choice(np.setdiff1d(np.arange(N_WORDS), own), k - n_own, replace=False)
        words = np.sort(np.concatenate([own, rest]))
        w = r.random(k) + 0.05
        w = w / w.sum()
        bows.append(OrderedDict(zip(words.tolist(), w.tolist())))
    conn, covis = [], []
    n = len(ids)
    for i in range(n):
        near = [j for j in range(max(0, i - 3), min(n_db, i + 4)) if j != i]
        same = [j for j in range(n_db) if j != i and place[j] == place[i]]
        conn.append(sorted(set(near[: int(r.integers(0, len(near) + 1))])))
        cand = list(dict.fromkeys(r.permutation(same + near).tolist()))
        covis.append(cand[: int(r.integers(3, 16))])
    return ids, bows, conn, covis, n_db


def make_ops(seed, n_db, n_all):
    r = np.random.default_rng(seed + 7)
    mins = [0.0, 0.01, 0.03, 0.05, 0.1, 0.15, 0.2, 0.3]
    ops = []
    double = {int(x) for x in r.choice(np.arange(5, n_db - 10), 2, replace=False)}
    for i in range(n_db):
        if i >= 6:
            ops.append((KO.OP_LOOP, i, mins[int(r.integers(len(mins)))]))
            if i % 9 == 0:  # the same query again: every keyframe already carries this mnId
                ops.append((KO.OP_LOOP, i, 0.0))
        ops.append((KO.OP_ADD, i, 0.0))
        if i in double:
            ops.append((KO.OP_ADD, i, 0.0))
        if i >= 10 and i % 7 == 0:
            ops.append((KO.OP_RELOC, int(r.integers(0, n_all)), 0.0))
        if i >= 12 and i % 8 == 0:
            ops.append((KO.OP_ERASE, int(r.integers(0, i - 2)), 0.0))
        if i == n_db // 2:  # the query-only stand-ins: mnId 0, the repeated id, then a relocalisation with it
            ops += [(KO.OP_LOOP, n_db, 0.0), (KO.OP_LOOP, n_db + 1, 0.05), (KO.OP_RELOC, n_db + 1, 0.0),
                    (KO.OP_RELOC, n_db, 0.0)]
    d = sorted(double)
    ops += [(KO.OP_ERASE, d[0], 0.0), (KO.OP_LOOP, n_db + 2, 0.0), (KO.OP_RELOC, n_db + 2, 0.0),
            (KO.OP_ERASE, d[0], 0.0), (KO.OP_LOOP, n_db + 3, 0.02), (KO.OP_RELOC, n_db + 3, 0.0),
            (KO.OP_ERASE, d[0], 0.0), (KO.OP_LOOP, n_db - 1, 0.1)]
    return ops


def flat(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return off, np.array([v for x in lists for v in x], np.int64)


def main():
    for name, seed in CASES:
        ids, bows, conn, covis, n_db = make_world(seed)
        ops = make_ops(seed, n_db, len(ids))
        b_off, b_word = flat([list(b.keys()) for b in bows])
        c_off, c_idx = flat(conn)
        v_off, v_idx = flat(covis)
        g = dict(kf_id=np.array(ids, np.int64), bow_off=b_off, bow_word=b_word.astype(np.int32),
                 bow_weight=np.array([v for b in bows for v in b.values()], np.float64), conn_off=c_off,
                 conn_idx=c_idx, covis_off=v_off, covis_idx=v_idx,
                 ops=np.array([(o, i) for o, i, _ in ops], np.int64), op_min=np.array([m for _, _, m in ops]))
        ref_kfs, ora_kfs = KO.world_from_golden(g), KO.world_from_golden(g)
        voc = RecordingVoc()
        ref_db, ora_db = KeyFrameDatabase(voc), KO.OracleKeyFrameDatabase()
        owner = {id(k.mBowVec): i for i, k in enumerate(ref_kfs)}
        n = len(ids)
        setter = np.full((2, n), -1, np.int64)  # query keyframe that last set mLoopScore / mRelocScore
        rec = dict(ret=[], ints=[], has=[], ls=[], rs=[], set_l=[], set_r=[])
        ora_ret = []
        KO.run_sequence(g, ora_db, ora_kfs, lambda q, got: ora_ret.append((got, KO.state_of(ora_kfs))))
        q_ops = [o for o in ops if o[0] in (KO.OP_LOOP, KO.OP_RELOC)]

        def on_query(q, got):
            for a, b in voc.pairs:
                setter[0 if q_ops[q][0] == KO.OP_LOOP else 1, owner[b]] = owner[a]
            voc.pairs.clear()
            ints, has, ls, rs = KO.state_of(ref_kfs)
            o_got, (o_ints, o_has, o_ls, o_rs) = ora_ret[q]
            assert got == o_got, (name, q, got, o_got)
            assert np.array_equal(ints, o_ints) and np.array_equal(has, o_has), (name, q)
            for k, v in zip(("ret", "ints", "has", "ls", "rs", "set_l", "set_r"),
                            (got, ints, has, ls, rs, setter[0].copy(), setter[1].copy())):
                rec[k].append(v)

        nq = KO.run_sequence(g, ref_db, ref_kfs, on_query)
        r_off, r_idx = flat(rec["ret"])
        g.update(ret_off=r_off, ret_idx=r_idx, state_int=np.array(rec["ints"]), has_loop_score=np.array(rec["has"]),
                 loop_score=np.array(rec["ls"]), reloc_score=np.array(rec["rs"]), loop_setter=np.array(rec["set_l"]),
                 reloc_setter=np.array(rec["set_r"]))
        np.savez_compressed(GOLD / f"kfdb_{name}.npz", **g)
        print(name, "ops", len(ops), "queries", nq, "non-empty", sum(1 for x in rec["ret"] if x),
              "max returned", max(len(x) for x in rec["ret"]), "bytes", (GOLD / f"kfdb_{name}.npz").stat().st_size)


if __name__ == "__main__":
    main()
