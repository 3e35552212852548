"""k_bow_score_many and k_bow_gate on the GPU: orbfe_kfdb_query_many, orbfe_kfdb_query_many_device and the
KeyFrameDatabase _many forms.

Dense rows against a loop of single-query launches, bit for bit (the two kernels share bow_pass); records against
the oracle of tests/kfdb_many_cases.py (kfdb_oracle.query_arrays plus int(max * ratio)).  Shapes are the smallest
that reach each boundary (tests/test_kfdb_many_cpu.py shows that they do): queries per tile, query lengths on
both sides of the LDS limit and of a tile's LDS budget, stored lengths around the 256-word pass, a second slot per
wave, a second compaction step, several chunks."""
import threading

import numpy as np
import pytest

import bow_cases as BC
import kfdb_many_cases as MC
import kfdb_oracle as KO

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def database_of(vecs, kf_capacity=1024, word_capacity=1 << 18):
    from pyorbslam_amd.kfdb import BowDatabase
    db = BowDatabase(kf_capacity, word_capacity)
    for s, v in enumerate(vecs):
        assert db.add(v if v is not None else {}) == s
        if v is None:
            db.erase(s)
    return db


def assert_dense_equals_loop(db, queries, recs, what=""):
    """recs' dense rows against one orbfe_kfdb_query launch per query."""
    for i, (q, r) in enumerate(zip(queries, recs)):
        common, first, score = db.query(q)
        assert np.array_equal(r["dense_common"], common), (what, i, "common")
        assert np.array_equal(r["dense_first"], first), (what, i, "first")
        assert np.array_equal(bits(r["dense_score"]), bits(score)), (what, i, "score")


def assert_records(recs, queries, vecs, ratio, exclude=None, hit_cap=None, what=""):
    for i, (q, r) in enumerate(zip(queries, recs)):
        ex = () if exclude is None or exclude[i] is None else exclude[i]
        MC.assert_record(r, MC.oracle_record(vecs, q, ratio, ex, hit_cap), f"{what} query {i} ratio {ratio}")


# ---- 1. dense rows and records ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    queries, vecs = MC.mixed_world()
    return queries, vecs, database_of(vecs)


@pytest.mark.parametrize("n_query", MC.q_counts())
def test_mixed_lengths_equal_single_launches_and_oracle(mixed, n_query):
    queries, vecs, db = mixed
    # the short calls take the long queries: 8 194 words alone, 8 192 + 8 191 overrunning the tile's LDS budget
    qs = {1: [queries[3]], 2: [queries[2], queries[1]]}.get(n_query, queries[:n_query])
    recs = db.query_many(qs, gate_ratio=0.8, dense=True)
    assert len(recs) == n_query and db.last_many_kernel_ms() > 0.0
    assert_dense_equals_loop(db, qs, recs, f"Q = {n_query}")
    assert_records(recs, qs, vecs, 0.8, what=f"Q = {n_query}")
    for r, q in zip(recs, qs):
        assert np.array_equal(bits(r["dense_score"][list(MC.MIXED_ERASED)]), bits([-0.0] * 3))
        assert np.array_equal(bits(r["dense_score"]), bits(KO.query_arrays(vecs, q)[2]))


def test_long_database_second_slot_per_wave_and_second_compaction_step():
    queries, vecs = MC.long_world()
    db = database_of(vecs, 1 << 14, 1 << 19)
    recs = db.query_many(queries, gate_ratio=0.0, dense=True)
    assert_dense_equals_loop(db, queries, recs, "long")
    assert_records(recs, queries, vecs, 0.0, what="long")
    step = MC.constants()["gate_step"]
    assert (recs[0]["slot"] < step).any() and (recs[0]["slot"] >= step).any()
    ex = [[8192], None] + [[0, 5, 8204]] * (len(queries) - 2)
    assert_records(db.query_many(queries, gate_ratio=0.8, exclude=ex), queries, vecs, 0.8, ex, what="long, gated")
    # hit_cap around a count that straddles the step
    n = recs[0]["n_hits"]
    for cap in (n - 1, n):
        assert_records(db.query_many(queries[:1], gate_ratio=0.0, hit_cap=cap), queries[:1], vecs, 0.0, hit_cap=cap)


def test_after_regrow_and_odd_weights():
    from pyorbslam_amd.kfdb import BowDatabase
    queries, vecs = MC.odd_world()
    r = np.random.default_rng(5)
    db = BowDatabase(2, 16)            # tiny hints: the arena and the slot table regrow while it fills
    mirror = []
    for v in vecs:
        mirror.append(None)
        db.erase(db.add(BC.random_vec(r, int(r.integers(1, 120)))))
        mirror.append(v)
        db.add(v)
    first = db.query_many(queries, gate_ratio=0.8, dense=True)   # a call in the middle of the growth
    before = db.stats()["regrows"]
    while db.stats()["regrows"] == before:
        v = BC.random_vec(r, 700)
        mirror.append(v)
        db.add(v)
    assert before > 0
    recs = db.query_many(queries, gate_ratio=0.8, dense=True)
    assert_dense_equals_loop(db, queries, recs, "regrown")
    assert_records(recs, queries, mirror, 0.8, what="regrown")
    n = len(first[0]["dense_common"])
    for a, b in zip(first, recs):
        assert np.array_equal(a["dense_common"], b["dense_common"][:n])
        assert np.array_equal(bits(a["dense_score"]), bits(b["dense_score"][:n]))


# ---- 2. gate and compaction ---------------------------------------------------------------------------------------
def test_gate_ties_exclusions_and_hit_caps():
    queries, vecs = MC.gate_world()
    db = database_of(vecs, 4, 64)
    n = len(vecs)
    for ratio in (0.0, 0.8, 0.5):       # 10 * 0.5 is an exact integer; at 0.8 three slots tie at the gate
        recs = db.query_many(queries, gate_ratio=ratio, dense=True)
        assert_records(recs, queries, vecs, ratio, what="planted")
        assert_dense_equals_loop(db, queries, recs, "planted")
    r = db.query_many(queries, gate_ratio=0.8)
    assert sorted(r[0]["common"].tolist()) == [9, 9, 10, 10] and r[0]["max_common"] == 10
    assert (r[1]["n_sharing"], r[1]["max_common"], r[1]["n_hits"], len(r[1]["slot"])) == (0, 0, 0, 0)
    for ex in ([[0, 6], None, [0]],                                  # the maximum is excluded: the gate moves
               [list(range(n)), list(range(n)), list(range(n))],     # every slot excluded
               [[4, 5], [2], None]):                                 # an erased and a non-sharing slot
        recs = db.query_many(queries, gate_ratio=0.8, exclude=ex, dense=True)
        assert_records(recs, queries, vecs, 0.8, ex, what=f"exclude {ex[0][:3]}")
        assert_dense_equals_loop(db, queries, recs, "excluded slots stay in the dense rows")
    assert db.query_many(queries, gate_ratio=0.8, exclude=[[0, 6], None, None])[0]["max_common"] == 9
    n_hits = r[0]["n_hits"]
    for cap in (0, n_hits - 1, n_hits):
        recs = db.query_many(queries, gate_ratio=0.8, hit_cap=cap)
        assert_records(recs, queries, vecs, 0.8, hit_cap=cap, what=f"hit_cap {cap}")
        assert recs[0]["n_hits"] == n_hits and len(recs[0]["slot"]) == cap
    # no hit_cap: one retry makes room for every hit
    from pyorbslam_amd import kfdb
    old, kfdb.HIT_CAP_FIRST = kfdb.HIT_CAP_FIRST, 2
    try:
        assert_records(db.query_many(queries, gate_ratio=0.0), queries, vecs, 0.0, what="retry")
    finally:
        kfdb.HIT_CAP_FIRST = old


# ---- 3. chunking ----------------------------------------------------------------------------------------------------
def test_chunked_calls_give_identical_bytes(mixed):
    queries, vecs, _ = mixed
    db = database_of(vecs)
    n_q, n = MC.constants()["tile"] + 1, len(vecs)
    qs = queries[:n_q]
    ex = [[1, 2]] + [None] * (n_q - 1)
    runs = []
    for limit in (1 << 30, -(-n_q // 2) * n * MC.ROW_BYTES, 0):
        db.set_scratch_limit(limit)
        runs.append(db.query_many(qs, gate_ratio=0.8, exclude=ex, dense=True))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.keys() == b.keys()
            for k in a:
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert_records(runs[2], qs, vecs, 0.8, ex, what="one query per chunk")


# ---- 4. the device entry --------------------------------------------------------------------------------------------
def test_query_bow_equals_query_many_on_fetched_arrays():
    import torch
    import vocab_synth as VS
    from pyorbslam_amd import synth
    from pyorbslam_amd.batch import StereoFrontEnd
    from pyorbslam_amd.kfdb import BowDatabase
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    t = VS.make_tree(seed=81, k=6, L=3, p_stop=0.2, p_dup=0.1, p_zero=0.1)
    v = TemplatedVocabulary(k=t["k"], L=t["L"]).from_arrays(t["parent"], t["is_leaf"], t["desc"], t["weight"])
    pairs = [synth.make_pair(s, 211, 157) for s in (3, 4)]
    imgs = torch.from_numpy(np.stack([im for p in pairs for im in p])).cuda()
    fe = StereoFrontEnd(211, 157, max_pairs=2, nfeatures=500)
    s = torch.cuda.current_stream()
    fe.enqueue(imgs, stream_ptr=s.cuda_stream)
    with pytest.raises(RuntimeError):
        fe.query_bow(BowDatabase())
    fe.bow(v, levels_up=1, side="both", stream_ptr=s.cuda_stream)
    stored = [fe.fetch_bow(i) for i in range(4)]
    db = BowDatabase(8, 4096)
    for a in stored:
        db.add_arrays(a.word, a.weight)
    db.add_arrays(np.zeros(0, np.int32), np.zeros(0))
    for side, n in (("left", 2), ("both", 4)):
        assert fe.bow(v, levels_up=1, side=side, stream_ptr=s.cuda_stream) == n
        arrs = [fe.fetch_bow(i) for i in range(n)]
        assert all(len(a.word) > 20 for a in arrs)
        ex = [[i] for i in range(n)]
        for kw in (dict(gate_ratio=0.8), dict(gate_ratio=0.0, exclude=ex), dict(gate_ratio=0.5, hit_cap=1)):
            got = fe.query_bow(db, stream_ptr=s.cuda_stream, dense=True, **kw)
            want = db.query_many_arrays([a.word for a in arrs], [a.weight for a in arrs], dense=True, **kw)
            assert len(got) == n
            for a, b in zip(got, want):
                assert a.keys() == b.keys()
                for k in a:
                    assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (side, k)
            assert all(r["n_sharing"] >= 1 for r in got)
    # a frame without words: an empty image pair has no keypoints
    blank = torch.zeros_like(imgs)
    blank[2:] = imgs[2:]
    fe.enqueue(blank, stream_ptr=s.cuda_stream)
    fe.bow(v, levels_up=1, side="left", stream_ptr=s.cuda_stream)
    assert len(fe.fetch_bow(0).word) == 0 and len(fe.fetch_bow(1).word) > 20
    got = fe.query_bow(db, stream_ptr=s.cuda_stream)
    assert (got[0]["n_sharing"], got[0]["max_common"], got[0]["n_hits"], len(got[0]["slot"])) == (0, 0, 0, 0)
    assert got[1]["n_hits"] >= 1 and 2 in got[1]["slot"]      # the frame itself is slot 2, above its own gate


# ---- 5. KeyFrameDatabase over the goldens -------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["w0", "w1", "w2"])
def test_keyframe_database_many_forms_over_golden_sequence(case):
    from pyorbslam_amd.kfdb import KeyFrameDatabase
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    g = KO.load_golden(case)
    skfs, kfs = KO.world_from_golden(g), KO.world_from_golden(g)
    single = []
    KO.run_sequence(g, KeyFrameDatabase(TemplatedVocabulary()), skfs,
                    lambda q, got: single.append((got, KO.state_of(skfs))))

    def on_group(qn, lists):
        for j, got in enumerate(lists):
            assert got == single[qn + j][0], (qn, j)
        last = qn + len(lists) - 1
        for mine, ref in zip(KO.state_of(kfs), single[last][1]):
            assert np.asarray(mine).tobytes() == np.asarray(ref).tobytes(), last
        KO.check_against_golden(g, kfs, last, lists[-1])

    assert MC.run_groups(g, KeyFrameDatabase(TemplatedVocabulary()), kfs, on_group) >= 3


# ---- 6. one database under four threads ---------------------------------------------------------------------------
def test_database_shared_by_threads():
    r = np.random.default_rng(92)
    base = BC.random_vec(r, 400)
    stored = [BC.overlapping_vec(r, base, int(r.integers(0, 300))) for _ in range(300)]
    sets = [[BC.overlapping_vec(r, base, n, 0.9) for n in lens] for lens in ((1, 40, 399), (200,), (0, 7, 90, 250), (64, 65))]
    want = [[(MC.oracle_record(stored, q, 0.8), KO.query_arrays(stored, q)) for q in qs] for qs in sets]
    # the writer's vectors share no word with anybody (ids above the vocabulary of the others)
    extra = [BC.with_weights(r, BC.N_WORDS + 1 + np.sort(r.choice(10 ** 6, 1500, replace=False))) for _ in range(20)]
    db = database_of(stored, 4, 64)
    errors = []

    def work(k):
        try:
            for it in range(12):
                if k == 0:
                    slot = db.add(extra[it])
                    if it % 2:
                        db.erase(slot)
                recs = db.query_many(sets[k], gate_ratio=0.8, dense=True)
                for q, (rec, (w_rec, w_dense)) in enumerate(zip(recs, want[k])):
                    MC.assert_record(rec, w_rec, f"thread {k} iteration {it} query {q}")
                    for name, x in zip(("dense_common", "dense_first", "dense_score"), w_dense):
                        if np.asarray(rec[name][:300]).tobytes() != np.asarray(x).tobytes():
                            errors.append((name, k, it, q))
        except Exception as e:  # reported below
            errors.append(("raised", k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:5]
    assert db.stats()["regrows"] > 0
