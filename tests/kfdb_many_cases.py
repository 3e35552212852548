"""Inputs and oracle of the many-query place-recognition tests (tests/test_gpu_kfdb_many.py) and of their CPU
pre-conditions (tests/test_kfdb_many_cpu.py).  Pure numpy / Python, deterministic by seed.

The oracle of a record is kfdb_oracle.query_arrays plus the word gate written as the reference writes it,
int(max * ratio) (KeyFrameDatabase.py:60-66).  The kernels' constants are read from the source text, so a retune
moves the cases with it."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

import bow_cases as BC
import kfdb_oracle as KO

ROW_BYTES = 16   # common + first + score of one (query, slot) in the handle's scratch


def constants() -> dict:
    k = BC.kernel_constants()
    return dict(tile=k["kBowTile"], waves=k["kBowManyWaves"], lds=k["kBowLdsWords"], tile_lds=k["kBowTileLdsWords"],
                max_blocks=k["kBowMaxBlocks"], pass_words=64 * k["kBowUnroll"],
                gate_step=k["kGateThreads"] * k["kGateItems"])


def q_counts() -> list:
    t = constants()["tile"]
    return sorted({1, 2, t - 1, t, t + 1, 2 * t + 1} - {0})


# ---- the oracle -------------------------------------------------------------------------------------------------
def oracle_record(vectors, q, ratio, excl=(), hit_cap=None, arrays=None) -> dict:
    """What one query's record must be.  vectors: one BoW dict per slot, None once erased."""
    common, first, score = arrays if arrays is not None else KO.query_arrays(vectors, q)
    n = len(vectors)
    live = np.array([v is not None for v in vectors], bool).reshape(n)
    ex = np.zeros(n, bool)
    ex[list(excl)] = True
    sharing = live & (common > 0)
    cand = sharing & ~ex
    mx = int(common[cand].max()) if cand.any() else 0
    gate = int(mx * ratio)
    hits = np.flatnonzero(cand & (common > gate))
    k = len(hits) if hit_cap is None else min(len(hits), hit_cap)
    h = hits[:k]
    return dict(n_sharing=int(sharing.sum()), max_common=mx, n_hits=len(hits), slot=h.astype(np.int32),
                common=common[h], first=first[h], score=score[h])


def assert_record(got: dict, want: dict, what="") -> None:
    for k in ("n_sharing", "max_common", "n_hits"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("slot", "common", "first"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])
    assert np.array_equal(np.asarray(got["score"]).view(np.uint64), np.asarray(want["score"]).view(np.uint64)), \
        (what, "score")
    assert np.all(np.diff(got["slot"]) > 0), (what, "ascending")


# ---- worlds -----------------------------------------------------------------------------------------------------
# kBowLdsWords = 8192 is the last length staged in LDS; in this order a tile of three or more queries holds an empty
# query, two whose ids together overrun the tile's LDS budget and one that is searched in global memory
QUERY_LENGTHS = [0, 8191, 8192, 8194, 1, 64, 65]
SMALL_LENGTHS = [0, 1, 2, 63, 64, 65, 300]
MIXED_ERASED = (3, 11, 20)


def sub_vec(r, base: dict, n: int) -> OrderedDict:
    """n of base's words, ascending, with weights of their own."""
    keys = np.fromiter(base.keys(), np.int64, len(base))
    return BC.with_weights(r, np.sort(r.choice(keys, n, replace=False)))


def mixed_world(seed: int = 61):
    """(queries, vectors with None at the erased slots).  2 * tile + 1 queries whose lengths cycle through
    QUERY_LENGTHS, all drawn from one 9 000-word pool, so one tile mixes empty, short, LDS-limit and global-search
    queries and 8 191 + 8 192 words overrun a tile's LDS budget; stored vectors of the lengths around the
    256-word pass (half and all of their words from the pool) and a few short ones."""
    r = np.random.default_rng(seed)
    pool = BC.random_vec(r, 9000)
    n_q = 2 * constants()["tile"] + 1
    queries = [sub_vec(r, pool, QUERY_LENGTHS[i % len(QUERY_LENGTHS)]) for i in range(n_q)]
    vecs = [BC.overlapping_vec(r, pool, n, share) for share in (0.5, 1.0) for n in BC.PASS_LENGTHS]
    vecs += [BC.overlapping_vec(r, pool, n, 0.7) for n in SMALL_LENGTHS]
    vecs += [OrderedDict(queries[1]), OrderedDict(queries[5])]
    for s in MIXED_ERASED:
        vecs[s] = None
    return queries, vecs


def long_q_count() -> int:
    """The fewest queries at which a wave of k_bow_score_many takes a second slot of BC.long_database(): the launch
    has max(1, kBowMaxBlocks // tiles) blocks of kBowManyWaves waves per tile."""
    c = constants()
    tiles = 1
    while max(1, c["max_blocks"] // tiles) * c["waves"] >= BC.LONG_SLOTS:
        tiles += 1
    return (tiles - 1) * c["tile"] + 1


def long_world():
    """BC.long_database() (8 205 slots) with long_q_count() queries: its own query, an empty one and sub-vectors
    of the query."""
    q, vecs, erased = BC.long_database()
    r = np.random.default_rng(71)
    n = long_q_count()
    queries = [q, OrderedDict()] + [sub_vec(r, q, int(r.integers(1, BC.LONG_NQ))) for _ in range(max(0, n - 2))]
    vecs = list(vecs)
    for s in erased:
        vecs[s] = None
    return queries[:n], vecs


def odd_world():
    q, vecs = BC.odd_weight_world()
    return [q, vecs[9], vecs[-9], OrderedDict()], list(vecs)


GATE_COMMON = [10, 9, 8, 8, 7, 0, 10, 3, 6, 5, 1, 8, 9, 0, 2]   # shared words of each planted slot with the query


def gate_world(seed: int = 81):
    """A 10-word query (ids 1000 * i) and one stored vector per entry of GATE_COMMON sharing exactly that many of
    its words (the first ones), padded with ids that are no multiple of 1000; slot 4 is erased afterwards (None).
    Second query: shares no word with anything.  Third: the first five words only."""
    r = np.random.default_rng(seed)
    qw = 1000 * np.arange(10)
    q = BC.with_weights(r, qw)
    vecs = []
    for c in GATE_COMMON:
        pad = 1000 * r.choice(500, 20, replace=False) + 20_000 + r.integers(1, 999, 20)
        vecs.append(BC.with_weights(r, np.sort(np.concatenate([qw[:c], pad]))))
    vecs[4] = None
    lonely = BC.with_weights(r, [500, 1500, 2500])
    return [q, lonely, BC.with_weights(r, qw[:5])], vecs


def chunk_count(limit: int, n_query: int, n_slots: int) -> int:
    per = max(1, limit // (n_slots * ROW_BYTES))
    return -(-n_query // min(per, n_query))


# ---- golden sequences through the _many forms ---------------------------------------------------------------------
def query_groups(g) -> list:
    """The golden's operations as a list of ("add" | "erase", kf index) and (OP_LOOP | OP_RELOC, [kf indices],
    [min scores], first query number): consecutive queries of one kind with no add or erase between them form
    one group."""
    out, qn = [], 0
    for (op, i), ms in zip(g["ops"].tolist(), g["op_min"].tolist()):
        if op in (KO.OP_ADD, KO.OP_ERASE):
            out.append(("add" if op == KO.OP_ADD else "erase", i))
            continue
        if out and out[-1][0] == op:
            out[-1][1].append(i)
            out[-1][2].append(ms)
        else:
            out.append((op, [i], [ms], qn))
        qn += 1
    return out


def run_groups(g, db, kfs, on_group) -> int:
    """Replay the golden with every query group through the _many forms; on_group(first query number, list of
    returned keyframe index lists).  Returns the number of groups of two or more queries."""
    index = {id(k): i for i, k in enumerate(kfs)}
    multi = 0
    for item in query_groups(g):
        if item[0] == "add":
            db.add(kfs[item[1]])
        elif item[0] == "erase":
            db.erase(kfs[item[1]])
        else:
            op, idx, ms, qn = item
            qs = [kfs[i] for i in idx]
            got = db.detect_loop_candidates_many(qs, ms) if op == KO.OP_LOOP else \
                db.detect_relocalization_candidates_many(qs)
            multi += len(idx) > 1
            on_group(qn, [[index[id(k)] for k in lst] for lst in got])
    return multi
