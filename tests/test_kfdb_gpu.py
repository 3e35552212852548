"""k_bow_score on the GPU: orbfe_kfdb_query, orbfe_bow_score and the KeyFrameDatabase drop-in against the
canonical-order oracle (tests/kfdb_oracle.py), bit for bit, and against the reference's recorded behaviour
(tests/golden/kfdb_*.npz).

Shapes are the smallest at which the kernel can go wrong: stored lengths around the 64-lane chunk (and the
32-lane half), query lengths around one chunk and on both sides of the LDS-resident limit (kBowLdsWords = 8192
in orbfe_kfdb.hip; 8193 takes the global-memory search).  A vector of distinct ids cannot be longer than its
vocabulary: under the 97-word vocabulary every length is capped at 97.
"""
import numpy as np
import pytest

import kfdb_oracle as KO

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300]
LDS_LIMIT = 8192
QUERY_LENGTHS = [0, 1, 64, 65, 1000, LDS_LIMIT + 1]
VOCABS = [97, 1_000_003]


def make_vec(r, n_words, n, top=False):
    n = min(n, n_words)
    if top and n:  # the id at the very top of the range
        w = np.append(np.sort(r.choice(n_words - 1, n - 1, replace=False)), n_words - 1)
    else:
        w = np.sort(r.choice(n_words, n, replace=False))
    v = r.random(len(w)) + 0.05
    return dict(zip(w.tolist(), (v / v.sum()).tolist()))


def world(n_words, nq, seed):
    """The query and ~70 stored vectors: lengths cycling through LENGTHS, then one with no shared word, one
    identical to the query and one strict subset of it."""
    r = np.random.default_rng(seed)
    q = make_vec(r, n_words, nq, top=True)
    vecs = [make_vec(r, n_words, LENGTHS[i % len(LENGTHS)], top=(i % 3 == 0)) for i in range(68)]
    rest = np.setdiff1d(np.arange(min(n_words, 5000)), np.fromiter(q.keys(), np.int64, len(q)))
    if len(rest):
        w = rest[:: max(1, len(rest) // 40)][:40]
        vecs.append(dict(zip(w.tolist(), np.full(len(w), 1.0 / len(w)).tolist())))
    vecs.append(dict(q))
    sub = dict(list(q.items())[1::2])
    vecs.append(sub)
    return q, vecs


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def assert_same(got, want, what=""):
    for g, w, name in zip(got, want, ("common", "first", "score")):
        g, w = (bits(g), bits(w)) if name == "score" else (np.asarray(g), np.asarray(w))
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, f"{what} {name}: slots {bad[:8].tolist()} got {got[2][bad[:4]] if name == 'score' else g[bad[:4]]}"


@pytest.mark.parametrize("nq", QUERY_LENGTHS)
@pytest.mark.parametrize("n_words", VOCABS)
def test_query_matches_oracle_bitwise(n_words, nq):
    from pyorbslam_amd.kfdb import BowDatabase
    q, vecs = world(n_words, nq, seed=n_words % 1000 + nq)
    db = BowDatabase(128, 1 << 14)
    for v in vecs:
        db.add(v)
    got = db.query(q)
    want = KO.query_arrays(vecs, q)
    assert_same(got, want, f"vocabulary {n_words}, query {nq}")
    if len(q):
        assert got[0][-2] == len(q) and got[1][-2] == min(q)           # the copy of the query
        assert got[2][-2] == 1.0 or abs(got[2][-2] - 1.0) < 1e-12       # L1-normalised: score 1
        assert got[0][-1] == len(q) // 2                                 # the strict subset
    if n_words > 97 or len(q) == 0:
        s = got[2][-3]
        assert got[0][-3] == 0 and got[1][-3] == -1 and s == 0.0 and np.signbit(s)  # no shared word: -0.0


def test_independent_of_order_erasures_and_growth():
    from pyorbslam_amd.kfdb import BowDatabase
    r = np.random.default_rng(77)
    q, vecs = world(3001, 200, seed=9)
    a = BowDatabase(128, 1 << 14)
    for v in vecs:
        a.add(v)
    ref = a.query(q)
    assert a.stats()["regrows"] == 0
    # another order, junk in between that is erased again, tiny capacity hints: the arena regrows and drops the junk
    b = BowDatabase(2, 16)
    where = {}
    junk = []
    for i in r.permutation(len(vecs)).tolist():
        junk.append(b.add(make_vec(r, 3001, int(r.integers(1, 200)))))
        where[i] = b.add(vecs[i])
        if len(junk) % 3 == 0:
            b.erase(junk.pop(0))
    mid = b.query(q)  # a query in the middle of the growth: the device copy is rebuilt afterwards
    for s in junk:
        b.erase(s)
    before, extra = b.stats()["regrows"], []
    while b.stats()["regrows"] == before:  # fill the arena until it regrows once more, now with erasures to drop
        extra.append(b.add(make_vec(r, 3001, 900)))
    st = b.stats()
    assert before > 0 and st["n_live"] == len(vecs) + len(extra)
    got = b.query(q)
    slots = np.array([where[i] for i in range(len(vecs))])
    assert_same([x[slots] for x in got], ref, "regrown database")
    assert_same([x[slots] for x in mid], ref, "before the last regrow")
    erased = np.setdiff1d(np.arange(st["n_slots"]), np.concatenate([slots, np.array(extra)]))
    assert len(erased) > 20
    assert np.all(got[0][erased] == 0) and np.all(got[1][erased] == -1)
    assert np.all(bits(got[2][erased]) == bits(-0.0))
    # erase in the plain handle too: neighbours keep their results
    a.erase(3)
    a.erase(len(vecs) - 2)
    again = a.query(q)
    keep = np.setdiff1d(np.arange(len(vecs)), [3, len(vecs) - 2])
    assert_same([x[keep] for x in again], [x[keep] for x in ref], "after erasing neighbours")
    assert again[0][3] == 0 and again[0][len(vecs) - 2] == 0


def test_empty_and_cleared_database():
    from pyorbslam_amd.kfdb import BowDatabase
    q, vecs = world(3001, 100, seed=4)
    db = BowDatabase(4, 64)
    assert all(len(x) == 0 for x in db.query(q))
    for v in vecs[:20]:
        db.add(v)
    first = db.query(q)
    assert db.last_kernel_ms() > 0.0
    db.clear()
    assert all(len(x) == 0 for x in db.query(q)) and db.last_kernel_ms() == 0.0
    for v in vecs[10:20]:
        db.add(v)
    assert_same(db.query(q), [x[10:20] for x in first], "after clear")
    assert_same(db.query({}), KO.query_arrays(vecs[10:20], {}), "empty query")


def test_score_many_equals_score_and_database():
    from pyorbslam_amd.kfdb import BowDatabase
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    voc = TemplatedVocabulary()
    q, vecs = world(3001, 300, seed=12)
    many = voc.score_many(q, vecs)
    assert isinstance(many, list) and all(type(x) is float for x in many)
    db = BowDatabase()
    for v in vecs:
        db.add(v)
    assert np.array_equal(bits(many), bits(db.query(q)[2]))
    assert np.array_equal(bits(many), bits(KO.query_arrays(vecs, q)[2]))
    for i in (0, 1, 5, 12, 30, len(vecs) - 3, len(vecs) - 2, len(vecs) - 1):
        one = voc.score(q, vecs[i])
        assert type(one) is float and bits(one) == bits(many[i])
    assert voc.score_many(q, []) == []
    s = voc.score({}, {})
    assert s == 0.0 and np.signbit(s)
    # unsorted plain dicts are accepted (the reference's l1_score takes any dict)
    rev = dict(reversed(list(vecs[12].items())))
    assert bits(voc.score(dict(reversed(list(q.items()))), rev)) == bits(many[12])


@pytest.mark.parametrize("case", ["w0", "w1", "w2"])
def test_keyframe_database_over_golden_sequence(case):
    """The whole drop-in: the reference's candidate lists and integer attributes exactly, scores within
    (n_common + 4) * 2^-52 of the reference's and bit-equal to the oracle's."""
    from pyorbslam_amd.kfdb import KeyFrameDatabase
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    g = KO.load_golden(case)
    kfs, okfs = KO.world_from_golden(g), KO.world_from_golden(g)
    ora = []
    KO.run_sequence(g, KO.OracleKeyFrameDatabase(), okfs, lambda q, got: ora.append((got, KO.state_of(okfs))))

    def on_query(q, got):
        KO.check_against_golden(g, kfs, q, got)
        o_got, (_, _, o_ls, o_rs) = ora[q]
        _, _, ls, rs = KO.state_of(kfs)
        assert got == o_got
        assert np.array_equal(bits(ls), bits(o_ls)) and np.array_equal(bits(rs), bits(o_rs))

    db = KeyFrameDatabase(TemplatedVocabulary())
    n = KO.run_sequence(g, db, kfs, on_query)
    assert n == len(ora)
    db.clear()
    assert db.detect_relocalization_candidates(kfs[5]) == []
