"""Place recognition without a GPU: the canonical-order oracle and the host replay of pyorbslam_amd.kfdb against
the reference's recorded behaviour (tests/golden/kfdb_*.npz, gen_golden_kfdb.py), and the host half of the
orbfe_kfdb library (storage, growth, argument checks).

Scores: ids and integer attributes are exact; a score may differ from the reference's by the summation order
only, |d| <= (n_common + 4) * 2^-52 (kfdb_oracle.score_bound).
"""
import numpy as np
import pytest

import kfdb_oracle as KO

CASES = ["w0", "w1", "w2"]


load, check_against_golden = KO.load_golden, KO.check_against_golden


@pytest.mark.parametrize("case", CASES)
def test_oracle_matches_reference(case):
    g = load(case)
    kfs = KO.world_from_golden(g)
    n = KO.run_sequence(g, KO.OracleKeyFrameDatabase(), kfs, lambda q, got: check_against_golden(g, kfs, q, got))
    assert n == len(g["ret_off"]) - 1 and n > 50
    ops = g["ops"][:, 0]
    assert (ops == KO.OP_RELOC).sum() > 5 and (ops == KO.OP_ERASE).sum() > 5


class OracleSlots:
    """Stands in for kfdb.BowDatabase: the same slots, result arrays computed by the oracle."""

    def __init__(self):
        self.vec = []

    def add(self, bv):
        self.vec.append(dict(bv))
        return len(self.vec) - 1

    def erase(self, s):
        assert self.vec[s] is not None
        self.vec[s] = None

    def clear(self):
        self.vec = []

    def query(self, bv):
        return KO.query_arrays(self.vec, bv)


def replay_database():
    from pyorbslam_amd import kfdb
    db = kfdb.KeyFrameDatabase.__new__(kfdb.KeyFrameDatabase)
    import threading
    db.mpVoc, db.mMutex, db._db, db._slot_kf, db._kf_slots = None, threading.Lock(), OracleSlots(), [], {}
    return db


@pytest.mark.parametrize("case", CASES)
def test_replay_matches_reference_and_oracle(case):
    """kfdb.replay_loop / replay_reloc (through KeyFrameDatabase's own add / erase bookkeeping) fed the oracle's
    result arrays: the reference's lists and integers, and the oracle's scores bit for bit."""
    g = load(case)
    kfs, okfs = KO.world_from_golden(g), KO.world_from_golden(g)
    ora = []
    KO.run_sequence(g, KO.OracleKeyFrameDatabase(), okfs, lambda q, got: ora.append((got, KO.state_of(okfs))))

    def on_query(q, got):
        check_against_golden(g, kfs, q, got)
        o_got, (o_int, o_has, o_ls, o_rs) = ora[q]
        _, _, ls, rs = KO.state_of(kfs)
        assert got == o_got
        assert np.array_equal(ls.view(np.uint64), o_ls.view(np.uint64))
        assert np.array_equal(rs.view(np.uint64), o_rs.view(np.uint64))

    KO.run_sequence(g, replay_database(), kfs, on_query)


def test_replay_clear_and_missing_erase():
    g = load("w0")
    kfs = KO.world_from_golden(g)
    db = replay_database()
    db.erase(kfs[0])  # never added: nothing happens, as in the reference
    for k in kfs[:10]:
        db.add(k)
    db.clear()
    assert db.detect_loop_candidates(kfs[20], 0.0) == [] and db.detect_relocalization_candidates(kfs[20]) == []
    assert kfs[3].mnLoopQuery == 0 and not hasattr(kfs[3], "mLoopScore")


def test_canonical_score_no_shared_word_is_negative_zero():
    s = KO.l1_canonical({1: 0.5, 2: 0.5}, {3: 1.0})
    assert s == 0.0 and np.signbit(s)


# ---- the library's host half: no device call -----------------------------------------------------------------

def vec(r, n_words, n):
    w = np.sort(r.choice(n_words, n, replace=False)).astype(np.int32)
    v = r.random(n) + 0.05
    return w, v / v.sum()


def test_add_refuses_unsorted_duplicate_negative():
    from pyorbslam_amd._lib import ORBFE_EINVAL, OrbfeError
    from pyorbslam_amd.kfdb import BowDatabase
    db = BowDatabase(4, 64)
    for bad in ([3, 2], [1, 1], [-1, 4], [0, 5, 5, 9]):
        with pytest.raises(OrbfeError) as e:
            db.add_arrays(np.array(bad, np.int32), np.full(len(bad), 0.5))
        assert e.value.code == ORBFE_EINVAL
    assert db.stats()["n_slots"] == 0
    assert db.add_arrays(np.zeros(0, np.int32), np.zeros(0)) == 0  # an empty vector is a vector
    assert db.add_arrays(np.array([0, 7], np.int32), np.array([0.5, 0.5])) == 1
    with pytest.raises(OrbfeError) as e:
        db.erase(2)
    assert e.value.code == ORBFE_EINVAL
    from pyorbslam_amd import _lib
    import ctypes as C
    for args in ((0, 16), (2, 0)):
        assert _lib.lib().orbfe_kfdb_create(args[0], args[1], C.byref(C.c_void_p())) == ORBFE_EINVAL


def test_stats_growth_and_stable_slots():
    from pyorbslam_amd._lib import ORBFE_ESTATE, OrbfeError
    from pyorbslam_amd.kfdb import BowDatabase
    r = np.random.default_rng(5)
    db = BowDatabase(2, 16)
    st = db.stats()
    assert (st["n_slots"], st["n_live"], st["live_words"], st["kf_capacity"], st["word_capacity"], st["regrows"]) == \
        (0, 0, 0, 2, 16, 0)
    lens, live = [], {}
    for i in range(40):
        w, v = vec(r, 500, int(r.integers(0, 30)))
        assert db.add_arrays(w, v) == i  # slot numbers are the insertion numbers, through every regrow
        lens.append(len(w))
        live[i] = len(w)
        if i % 5 == 4:
            db.erase(i - 2)
            del live[i - 2]
            with pytest.raises(OrbfeError) as e:
                db.erase(i - 2)
            assert e.value.code == ORBFE_ESTATE
        st = db.stats()
        assert st["n_slots"] == i + 1 and st["n_live"] == len(live) and st["live_words"] == sum(live.values())
        assert st["kf_capacity"] >= i + 1 and st["word_capacity"] >= st["live_words"]
    assert st["regrows"] > 0
    # capacities are the hints doubled
    assert st["kf_capacity"] == 64 and st["word_capacity"] & (st["word_capacity"] - 1) == 0
    db.clear()
    st2 = db.stats()
    assert (st2["n_slots"], st2["n_live"], st2["live_words"]) == (0, 0, 0)
    assert st2["kf_capacity"] == st["kf_capacity"] and st2["word_capacity"] == st["word_capacity"]
    assert db.add_arrays(*vec(r, 500, 5)) == 0


def test_query_checks_arguments_before_any_device_call():
    from pyorbslam_amd import _lib
    from pyorbslam_amd.kfdb import BowDatabase
    db = BowDatabase(2, 16)
    w = np.array([4, 2], np.int32)
    v = np.array([0.5, 0.5])
    out = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.float64)
    rc = _lib.lib().orbfe_kfdb_query(db._h, _lib.ptr(w), _lib.ptr(v), 2, *(_lib.ptr(o) for o in out), 4)
    assert rc == _lib.ORBFE_EINVAL
    db.add_arrays(np.array([1], np.int32), np.array([1.0]))
    db.add_arrays(np.array([1], np.int32), np.array([1.0]))
    w.sort()
    rc = _lib.lib().orbfe_kfdb_query(db._h, _lib.ptr(w), _lib.ptr(v), 2, *(_lib.ptr(o) for o in out), 1)
    assert rc == _lib.ORBFE_ECAPACITY
    # an empty database answers without a device
    db.clear()
    c, f, s = db.query_arrays(w, v)
    assert len(c) == len(f) == len(s) == 0 and db.last_kernel_ms() == 0.0


# ---- TemplatedVocabulary.score's selection ------------------------------------------------------------------

def test_unknown_scoring_raises_type_error():
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    with pytest.raises(TypeError):
        TemplatedVocabulary(scoring="nonsense").score({}, {})
    with pytest.raises(TypeError):
        TemplatedVocabulary(scoring="nonsense").score_many({}, [{}])


def test_scoring_function_survives_load(tmp_path):
    """load_from_text_file overwrites .scoring with the header integer; the function chosen by the constructor
    string stays (TemplatedVocabulary.py:39-40, 55)."""
    import vocab_synth as VS
    from pyorbslam_amd import vocabulary
    path = tmp_path / "voc.txt"
    VS.write_text(VS.make_tree(seed=1, k=3, L=2), path)
    voc = vocabulary.TemplatedVocabulary()
    assert voc.scoring == "L1_NORM" and voc.scoring_object is vocabulary._l1_score
    assert voc.load_from_text_file(str(path))
    assert isinstance(voc.scoring, int)
    assert voc.scoring_object is vocabulary._l1_score
    dot = vocabulary.TemplatedVocabulary(scoring="DOT_PRODUCT")
    assert dot.load_from_text_file(str(path))
    assert dot.score({1: 0.5, 2: 0.5}, {2: 0.5, 3: 0.5}) == 0.25
    assert dot.score_many({1: 0.5, 2: 0.5}, [{2: 0.5}, {7: 1.0}]) == [0.25, 0]


def test_host_scorings_match_their_definitions():
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    a, b = {1: 0.25, 2: 0.75}, {2: 0.5, 3: 0.5}
    assert TemplatedVocabulary(scoring="L2_NORM").score(a, b) == 1.0 - np.sqrt(1.0 - 0.375)
    assert TemplatedVocabulary(scoring="CHI_SQUARE").score(a, b) == 2.0 * (0.375 / 1.25)
    assert TemplatedVocabulary(scoring="BHATTACHARYYA").score(a, b) == np.sqrt(0.375)
    eps = np.log(np.finfo(float).eps)
    assert TemplatedVocabulary(scoring="KL").score(a, b) == 0.25 * (np.log(0.25) - eps) + 0.75 * np.log(0.75 / 0.5)
