"""The many-query database call without a GPU: every refusal of orbfe_kfdb_query_many / _many_device comes back
before any device call, the empty database and n_query = 0 answer on this host, the ABI table agrees with the
header, and the inputs of tests/test_gpu_kfdb_many.py reach the boundaries they claim (tile, pass, LDS limit,
second slot per wave, compaction step, chunk)."""
import ctypes as C
import re

import numpy as np
import pytest

import bow_cases as BC
import kfdb_many_cases as MC
import kfdb_oracle as KO
from conftest import ROOT

NEW = ["orbfe_kfdb_query_many", "orbfe_kfdb_query_many_device", "orbfe_kfdb_set_scratch_limit",
       "orbfe_kfdb_many_last_ms"]


# ---- the ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_resolve_and_abi_is_still_9():
    from pyorbslam_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.orbfe_abi_version() == 9 == _lib.ORBFE_ABI_VERSION
    assert C.sizeof(_lib.KfdbManyOut) == 10 * C.sizeof(C.c_void_p)


def test_table_and_header_agree():
    from pyorbslam_amd import _lib
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_kfdb_many_out \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in _lib.KfdbManyOut._fields_]
    assert int(re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1)) == 9


# ---- refusals, before any device call -----------------------------------------------------------------------------
class Call:
    """One orbfe_kfdb_query_many call over host arrays, every argument replaceable."""

    def __init__(self, db, n_query=2, hit_cap=4, n_slots=None):
        self.db = db
        self.off = np.array([0, 2, 3], np.int64)
        self.word = np.array([1, 5, 2], np.int32)
        self.weight = np.array([0.5, 0.5, 1.0])
        self.n_query, self.hit_cap, self.ratio = n_query, hit_cap, 0.8
        self.excl_off, self.excl_slot = None, None
        n = db.stats()["n_slots"] if n_slots is None else n_slots
        self.stride = n
        self.per = np.full((3, 2), 77, np.int32)
        self.hit = np.zeros((3, 2, 8), np.int32)
        self.hit_score = np.zeros((2, 8))
        self.dense = [np.zeros((2, max(n, 1)), np.int32), np.zeros((2, max(n, 1)), np.int32),
                      np.zeros((2, max(n, 1)))]
        self.with_dense = False

    def out(self):
        from pyorbslam_amd import _lib
        d = self.dense if self.with_dense else [None] * 3
        return _lib.KfdbManyOut(*(None if a is None else a.ctypes.data for a in (
            self.per[0], self.per[1], self.per[2], self.hit[0], self.hit[1], self.hit[2], self.hit_score, *d)))

    def host(self, out="own"):
        from pyorbslam_amd import _lib
        o = self.out() if out == "own" else out
        return _lib.lib().orbfe_kfdb_query_many(
            self.db._h, _lib.ptr(self.off), _lib.ptr(self.word), _lib.ptr(self.weight), self.n_query,
            _lib.ptr(self.excl_off), _lib.ptr(self.excl_slot), self.ratio, self.hit_cap, self.stride,
            None if o is None else C.byref(o))

    def device(self, bow="own", stride=8):
        """The device entry with pointers that are never followed: every refusal comes first."""
        from pyorbslam_amd import _lib
        b = _lib.BowOut(n_words=8, bow_word=8, bow_weight=8) if bow == "own" else bow
        o = self.out()
        return _lib.lib().orbfe_kfdb_query_many_device(
            self.db._h, None if b is None else C.byref(b), stride, self.n_query, _lib.ptr(self.excl_off),
            _lib.ptr(self.excl_slot), self.ratio, self.hit_cap, self.stride, C.byref(o), None)


def filled(n=3):
    from pyorbslam_amd.kfdb import BowDatabase
    db = BowDatabase(2, 16)
    for i in range(n):
        db.add_arrays(np.array([1, 2 + i], np.int32), np.array([0.5, 0.5]))
    return db


def bad_host_calls(db):
    """(what, call) for every refusal with ORBFE_EINVAL of the host entry."""
    def mk(**kw):
        c = Call(db)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    i64, i32 = (lambda *a: np.array(a, np.int64)), (lambda *a: np.array(a, np.int32))
    return [
        ("descending ids", mk(word=i32(5, 1, 2))),
        ("duplicate ids", mk(word=i32(5, 5, 2))),
        ("negative id", mk(word=i32(-1, 5, 2))),
        ("q_off not from 0", mk(off=i64(1, 2, 3))),
        ("q_off descending", mk(off=i64(0, 3, 2))),
        ("negative n_query", mk(n_query=-1)),
        ("ratio 1", mk(ratio=1.0)),
        ("ratio below 0", mk(ratio=-0.1)),
        ("ratio nan", mk(ratio=float("nan"))),
        ("negative hit_cap", mk(hit_cap=-1)),
        ("negative stride", mk(stride=-1)),
        ("excl_off not from 0", mk(excl_off=i64(1, 1, 1), excl_slot=i32(0))),
        ("excl_off descending", mk(excl_off=i64(0, 2, 1), excl_slot=i32(0, 1))),
        ("exclusions descending", mk(excl_off=i64(0, 2, 2), excl_slot=i32(1, 0))),
        ("exclusions repeated", mk(excl_off=i64(0, 2, 2), excl_slot=i32(1, 1))),
        ("exclusion at n_slots", mk(excl_off=i64(0, 1, 2), excl_slot=i32(0, 3))),
        ("negative exclusion", mk(excl_off=i64(0, 1, 2), excl_slot=i32(-1, 0))),
    ]


def test_host_entry_refuses_before_any_device_call():
    from pyorbslam_amd import _lib
    db = filled()
    for what, c in bad_host_calls(db):
        assert c.host() == _lib.ORBFE_EINVAL, what
        assert np.all(c.per == 77), what
    c = Call(db)
    assert c.host(out=None) == _lib.ORBFE_EINVAL
    o = c.out()
    o.n_hits = None
    assert c.host(out=o) == _lib.ORBFE_EINVAL
    o = c.out()
    o.hit_first = None
    assert c.host(out=o) == _lib.ORBFE_EINVAL
    # dense rows shorter than the slot table: ECAPACITY, as orbfe_kfdb_query; without a dense pointer the stride
    # is not looked at
    c = Call(db)
    c.with_dense, c.stride = True, 2
    assert c.host() == _lib.ORBFE_ECAPACITY
    assert _lib.lib().orbfe_kfdb_query_many(None, None, None, None, 0, None, None, 0.0, 0, 0, None) == _lib.ORBFE_EINVAL
    assert _lib.lib().orbfe_kfdb_set_scratch_limit(db._h, -1) == _lib.ORBFE_EINVAL
    assert _lib.lib().orbfe_kfdb_many_last_ms(db._h, None) == _lib.ORBFE_EINVAL


def test_device_entry_refuses_before_any_device_call():
    from pyorbslam_amd import _lib
    db = filled()
    c = Call(db)
    for what, kw in (("ratio", dict(ratio=1.0)), ("hit_cap", dict(hit_cap=-2)), ("n_query", dict(n_query=-1)),
                     ("exclusion", dict(excl_off=np.array([0, 1, 2], np.int64), excl_slot=np.array([0, 3], np.int32)))):
        c = Call(db)
        for k, v in kw.items():
            setattr(c, k, v)
        assert c.device() == _lib.ORBFE_EINVAL, what
    assert Call(db).device(bow=None) == _lib.ORBFE_EINVAL
    assert Call(db).device(bow=_lib.BowOut(n_words=8)) == _lib.ORBFE_EINVAL
    assert Call(db).device(stride=-1) == _lib.ORBFE_EINVAL
    c = Call(db)
    c.with_dense, c.stride = True, 1
    assert c.device() == _lib.ORBFE_ECAPACITY


def test_empty_database_and_no_query_answer_without_a_device():
    from pyorbslam_amd import _lib
    from pyorbslam_amd.kfdb import BowDatabase
    db = BowDatabase(2, 16)
    c = Call(db)
    assert c.host() == 0 and np.all(c.per == 0)
    c = Call(db)
    assert c.device() == 0 and np.all(c.per == 0)
    recs = db.query_many([{1: 0.5, 4: 0.5}, {}], gate_ratio=0.8, dense=True)
    assert len(recs) == 2 and db.last_many_kernel_ms() == 0.0
    for r in recs:
        assert (r["n_sharing"], r["max_common"], r["n_hits"]) == (0, 0, 0)
        assert all(len(r[k]) == 0 for k in ("slot", "common", "first", "score", "dense_common", "dense_score"))
    full = filled()
    c = Call(full, n_query=0)
    assert c.host() == 0 and np.all(c.per == 77)       # nothing is written for no query
    assert c.device() == 0
    assert full.query_many_arrays([], []) == [] and full.last_many_kernel_ms() == 0.0
    db.set_scratch_limit(0)
    db.set_scratch_limit(1 << 30)
    with pytest.raises(ValueError):
        full.query_many([{1: 1.0}], exclude=[[0], [1]])
    with pytest.raises(_lib.OrbfeError) as e:
        full.query_many([{1: 1.0}], exclude=[[7]])
    assert e.value.code == _lib.ORBFE_EINVAL


# ---- the oracle's gate ------------------------------------------------------------------------------------------
def test_oracle_gate_keeps_gate_plus_one_and_drops_gate():
    qs, vecs = MC.gate_world()
    common = KO.query_arrays(vecs, qs[0])[0]
    want = np.array(MC.GATE_COMMON)
    want[4] = 0                                              # the erased slot
    assert common.tolist() == want.tolist()
    r = MC.oracle_record(vecs, qs[0], 0.8)
    assert r["max_common"] == 10 and int(10 * 0.8) == 8
    assert sorted(r["common"].tolist()) == [9, 9, 10, 10]    # 9 = gate + 1 stays, the three 8 = gate go
    assert r["n_sharing"] == sum(c > 0 for c in want) and r["n_hits"] == 4
    half = MC.oracle_record(vecs, qs[0], 0.5)                # 10 * 0.5 is the integer 5
    assert 6 in half["common"] and 5 not in half["common"] and half["common"].min() == 6
    assert MC.oracle_record(vecs, qs[0], 0.0)["n_hits"] == r["n_sharing"]
    # exclusions: removing both slots with 10 moves the gate to int(9 * 0.8) = 7; the 8s come back
    ex = MC.oracle_record(vecs, qs[0], 0.8, excl=[0, 6])
    assert ex["max_common"] == 9 and sorted(ex["common"].tolist()) == [8, 8, 8, 9, 9] and ex["n_sharing"] == r["n_sharing"]
    everything = MC.oracle_record(vecs, qs[0], 0.8, excl=range(len(vecs)))
    assert (everything["max_common"], everything["n_hits"]) == (0, 0) and everything["n_sharing"] == r["n_sharing"]
    lonely = MC.oracle_record(vecs, qs[1], 0.8)
    assert (lonely["n_sharing"], lonely["max_common"], lonely["n_hits"]) == (0, 0, 0)
    assert MC.oracle_record(vecs, qs[0], 0.8, hit_cap=3)["slot"].tolist() == r["slot"][:3].tolist()
    assert MC.oracle_record(vecs, qs[0], 0.8, hit_cap=3)["n_hits"] == 4
    # the device's expression is the reference's
    for mx in range(0, 3000):
        for ratio in (0.8, 0.5, 0.75, 0.1):
            assert int(mx * ratio) == int(np.int32(np.float64(mx) * np.float64(ratio)))


# ---- the cases reach their boundaries -----------------------------------------------------------------------------
def test_cases_reach_tile_pass_lds_and_budget_boundaries():
    c = MC.constants()
    t = c["tile"]
    assert MC.q_counts() == sorted({1, 2, t - 1, t, t + 1, 2 * t + 1}) and 3 <= t <= 64
    queries, vecs = MC.mixed_world()
    assert len(queries) == 2 * t + 1
    lens = [len(q) for q in queries]
    assert c["lds"] == 8192 and {0, 1, c["lds"] - 1, c["lds"], c["lds"] + 2} <= set(lens)
    first_tile = lens[:t]
    assert 0 in first_tile and max(first_tile) > c["lds"] and c["lds"] in first_tile    # one tile mixes them
    # the tile's packed ids overrun its LDS budget: a query that alone would be staged is searched in global memory
    used, spilled = 0, []
    for n in first_tile:
        if n <= c["lds"] and used + n <= c["tile_lds"]:
            used += n
        elif n <= c["lds"]:
            spilled.append(n)
    assert spilled and used <= c["tile_lds"]
    stored = [len(v) for v in vecs if v is not None]
    p = c["pass_words"]
    assert {p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1} <= set(stored) and 0 in stored
    assert all(vecs[s] is None for s in MC.MIXED_ERASED)
    # every query shares words with some stored vector, and the LDS-limit queries with the long ones
    for q in queries:
        if len(q):
            assert KO.query_arrays(vecs, q)[0].max() > 0


def test_long_world_takes_a_second_slot_and_straddles_a_compaction_step():
    c = MC.constants()
    queries, vecs = MC.long_world()
    n_q = MC.long_q_count()
    assert len(queries) == n_q and len(vecs) == BC.LONG_SLOTS
    tiles = -(-n_q // c["tile"])
    waves = max(1, c["max_blocks"] // tiles) * c["waves"]
    assert waves < BC.LONG_SLOTS <= 2 * waves           # some waves take a second slot, none a third
    one_less = -(-(n_q - 1) // c["tile"])
    assert n_q == 1 or max(1, c["max_blocks"] // one_less) * c["waves"] >= BC.LONG_SLOTS
    assert any(v is None for v in vecs)
    # hits on both sides of the first compaction step, at ratio 0 and at ratio 0.8
    step = c["gate_step"]
    assert step < BC.LONG_SLOTS
    r0 = MC.oracle_record(vecs, queries[0], 0.0)
    assert (r0["slot"] < step).sum() > 1000 and (r0["slot"] >= step).sum() > 1000
    assert MC.oracle_record(vecs, queries[0], 0.8)["slot"].tolist() == [8192]       # the query's own copy
    sub = MC.oracle_record(vecs, queries[2], 0.8)
    assert sub["n_hits"] >= 1 and sub["max_common"] == len(queries[2])


def test_chunk_limits_give_one_two_and_q_chunks():
    queries, vecs = MC.mixed_world()
    n_q, n = MC.constants()["tile"] + 1, len(vecs)
    assert MC.chunk_count(1 << 30, n_q, n) == 1
    assert MC.chunk_count(-(-n_q // 2) * n * MC.ROW_BYTES, n_q, n) == 2
    assert MC.chunk_count(0, n_q, n) == n_q and MC.chunk_count(n * MC.ROW_BYTES, n_q, n) == n_q


class OracleManySlots:
    """Stands in for kfdb.BowDatabase under KeyFrameDatabase: dense rows from the oracle."""

    def __init__(self):
        self.vec = []

    def add(self, bv):
        self.vec.append(dict(bv))
        return len(self.vec) - 1

    def erase(self, s):
        self.vec[s] = None

    def query(self, bv):
        return KO.query_arrays(self.vec, bv)

    def query_many(self, bvs, hit_cap=None, dense=False):
        assert dense and hit_cap == 0
        return [dict(zip(("dense_common", "dense_first", "dense_score"), KO.query_arrays(self.vec, bv))) for bv in bvs]


@pytest.mark.parametrize("case", ["w0", "w1", "w2"])
def test_many_forms_replay_equals_single_calls(case):
    """KeyFrameDatabase.detect_*_candidates_many over the oracle's rows: the single-call run's lists and state."""
    import threading
    from pyorbslam_amd import kfdb
    g = KO.load_golden(case)

    def database():
        db = kfdb.KeyFrameDatabase.__new__(kfdb.KeyFrameDatabase)
        db.mpVoc, db.mMutex, db._db, db._slot_kf, db._kf_slots = None, threading.Lock(), OracleManySlots(), [], {}
        return db

    skfs, kfs = KO.world_from_golden(g), KO.world_from_golden(g)
    single = []
    KO.run_sequence(g, database(), skfs, lambda q, got: single.append((got, KO.state_of(skfs))))

    def on_group(qn, lists):
        for j, got in enumerate(lists):
            assert got == single[qn + j][0], (qn, j)
        last = qn + len(lists) - 1
        for mine, ref in zip(KO.state_of(kfs), single[last][1]):
            assert np.array_equal(mine, ref), last
        KO.check_against_golden(g, kfs, last, lists[-1])

    multi = MC.run_groups(g, database(), kfs, on_group)
    assert multi >= 3, "the golden must hold consecutive queries with no add or erase between them"
    assert sum(len(x[1]) for x in MC.query_groups(g) if x[0] not in ("add", "erase")) == len(single)
