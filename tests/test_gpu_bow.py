"""The bag-of-words path at its loop boundaries on the GPU: k_vocab_descend on nodes wider than one 32-lane pass
(against the reference's own outputs, tests/golden/vocab_wide.npz, and VocabOracle) and k_bow_score where a wave
takes a second slot, a stored vector a second 256-word pass and the query the last LDS-resident lengths (bit for
bit against tests/kfdb_oracle.py).  The inputs come from tests/bow_cases.py; tests/test_bow_cases_cpu.py shows
that they reach what they aim at."""
import ctypes as C
import threading

import numpy as np
import pytest

import bow_cases as BC
import kfdb_oracle as KO
import vocab_synth as VS
from oracle.vocab_oracle import VocabOracle
from test_kfdb_gpu import assert_same, bits
from test_vocab import golden_outputs, same

pytestmark = pytest.mark.gpu


def oracle_of(t):
    return VocabOracle(t["parent"], t["is_leaf"], t["desc"], t["weight"], t["L"])


def native_of(t):
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    return TemplatedVocabulary(k=t["k"], L=t["L"]).from_arrays(t["parent"], t["is_leaf"], t["desc"], t["weight"])


def assert_descend(v, o, q, levels_up, what=""):
    word, node, w = v.descend(q, levels_up)
    want = [o.descend(x, o.L - levels_up) for x in q]
    got = list(zip(word.tolist(), node.tolist(), w.tolist()))
    bad = [i for i, (g, x) in enumerate(zip(got, want)) if g != x]
    assert not bad, f"{what}: {len(bad)} of {len(q)} descents differ, first {bad[:5]}: {got[bad[0]]} != {want[bad[0]]}"


# ---- 1. wide nodes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    z, tree, q = BC.wide_golden()
    return z, tree, q


def test_wide_transform_golden(wide, tmp_path):
    """The text loader's tree and one launch per levels_up against the reference's BoW and feature vectors."""
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    z, tree, q = wide
    path = tmp_path / "wide.txt"
    VS.write_text(tree, path)
    v = TemplatedVocabulary()
    assert v.load_from_text_file(path) and v.info().max_children == 300
    for lu in (0, 1, 2):
        got = v.transform(q, lu)
        same(got, *golden_outputs(z, lu))
        assert type(got[0]).__name__ == str(z[f"bv_type_{lu}"])


def test_wide_transform_many_golden(wide):
    """Several frames in one launch: the concatenation's per-frame results, and the whole set as one frame
    against the golden."""
    z, tree, q = wide
    v, o = native_of(tree), oracle_of(tree)
    for lu in (0, 1, 2):
        same(v.transform_many([q[:0], q], lu)[1], *golden_outputs(z, lu))
    frames = [q[:7], q[7:8], q[8:8], q[8:1000], q[1000:1003], q[1003:]]
    for f, got in zip(frames, v.transform_many(frames, 1)):
        want = o.transform(f, 1)
        assert list(got[0].items()) == list(want[0].items()) and list(got[1].items()) == list(want[1].items())


def test_wide_descend_every_query(wide):
    _, tree, q = wide
    v, o = native_of(tree), oracle_of(tree)
    for lu in (0, 1):
        assert_descend(v, o, q, lu, f"wide tree, levels_up {lu}")


# ---- 2. the largest fan-out -------------------------------------------------------------------------------------
def test_flat_tree_65535_children():
    """One node with 65 535 children: the child position fills the key's low 16 bits (2 048 passes per descent);
    equal leaves on both sides of 2^15 and at (3, 65 534), copies and near copies of leaves as queries."""
    t = BC.flat_tree(61)
    q, _ = BC.flat_queries(t, 62)
    v = native_of(t)
    assert v.info().max_children == 65535
    assert_descend(v, oracle_of(t), q, 0, "65 535 leaves under the root")


# ---- 3. descent edges -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    t = BC.ragged_tree()
    return t, oracle_of(t), VS.query_descriptors(t, 81, 120)


def test_descend_block_tail(ragged):
    """n = 1..17: the last block holds 1..8 descriptors (8 per 256-thread block), the last wave one or two."""
    t, o, q = ragged
    v = native_of(t)
    for n in range(1, 18):
        assert_descend(v, o, q[40:40 + n], 2, f"{n} descriptors")
    assert all(len(x) == 0 for x in v.descend(q[:0], 2))


def test_levels_up_outside_the_tree(ragged):
    """levels_up = -1 .. L + 1, i.e. a node level of L + 1, L, .., 0, -1: a level no descent has never matches,
    so every feature keeps node id 0."""
    t, o, q = ragged
    v = native_of(t)
    L = t["L"]
    for lu in range(-1, L + 2):
        got = v.transform(q, lu)
        want = o.transform(q, lu)
        assert list(got[0].items()) == list(want[0].items()) and list(got[1].items()) == list(want[1].items()), lu
        if lu in (-1, L, L + 1):
            assert list(got[1]) == [0]
            assert np.all(v.descend(q, lu)[1] == -1)


def test_mismatched_leaf_flags():
    t = BC.mismatched_tree(71)
    q = VS.query_descriptors(t, 72, 600)
    v, o = native_of(t), oracle_of(t)
    assert np.array_equal(v.node_arrays()["word_id"], o.word)
    for lu in (1, 2):
        assert_descend(v, o, q, lu, "mismatched flags")
        got, want = v.transform(q, lu), o.transform(q, lu)
        assert list(got[0].items()) == list(want[0].items()) and list(got[1].items()) == list(want[1].items())


def test_unloaded_vocabulary_transforms_to_nothing(ragged):
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    _, _, q = ragged
    v = TemplatedVocabulary()
    assert v.transform(q) == ({}, {})
    word, node, w = v.descend(q, 4)
    assert not word.any() and not w.any() and np.all(node == -1)


def test_transform_device_alignment_and_empty(ragged):
    """The device entry point reads descriptors as 16-byte vectors: the host refuses a pointer that is not 16-byte
    aligned before any launch, takes one 16 bytes into a larger buffer, and accepts n = 0."""
    import torch
    from pyorbslam_amd._lib import ORBFE_EINVAL, lib
    t, o, q = ragged
    v = native_of(t)
    n = len(q)
    buf = torch.zeros(n * 32 + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[16:16 + n * 32] = torch.from_numpy(q.reshape(-1)).cuda()
    word = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    node = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()

    def run(offset, count):
        return lib().orbfe_vocab_transform_device(v._handle(), C.c_void_p(buf.data_ptr() + offset), count, 2,
                                                  C.c_void_p(word.data_ptr()), C.c_void_p(node.data_ptr()),
                                                  C.c_void_p(w.data_ptr()), C.c_void_p(s.cuda_stream))

    assert run(8, n) == ORBFE_EINVAL and b"aligned" in lib().orbfe_last_error()
    assert run(16, 0) == 0
    s.synchronize()
    assert bool((word == -7).all()) and bool((node == -7).all()) and bool((w == -7.0).all())   # nothing ran
    assert run(16, n) == 0
    s.synchronize()
    hw, hn, hwt = v.descend(q, 2)
    assert np.array_equal(word.cpu().numpy(), hw) and np.array_equal(node.cpu().numpy(), hn)
    assert np.array_equal(bits(w.cpu().numpy()), bits(hwt))
    assert_descend(v, o, q, 2, "host entry point")


# ---- 4. k_bow_score ---------------------------------------------------------------------------------------------
def database_of(vecs, kf_capacity=128, word_capacity=1 << 14):
    from pyorbslam_amd.kfdb import BowDatabase
    db = BowDatabase(kf_capacity, word_capacity)
    for v in vecs:
        db.add(v)
    return db


def test_long_database_second_slot_per_wave():
    """8 205 slots under 8 192 waves: thirteen waves score a second vector, after the first one's counters."""
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    q, vecs, erased = BC.long_database()
    db = database_of(vecs, 16384, 1 << 19)
    assert db.stats()["regrows"] == 0
    full = db.query(q)
    assert_same(full, KO.query_arrays(vecs, q), "8 205 live slots")
    for s in erased:
        db.erase(s)
    live = [None if s in set(erased) else v for s, v in enumerate(vecs)]
    got = db.query(q)
    assert_same(got, KO.query_arrays(live, q), "with erased slots")
    e = np.array(erased)
    assert np.all(got[0][e] == 0) and np.all(got[1][e] == -1) and np.all(bits(got[2][e]) == bits(-0.0))
    assert got[0][8192] == 200 and got[1][8192] == min(q)
    assert all(got[0][s] > 0 for s in BC.LONG_KEEP)
    # orbfe_bow_score: the same kernel under the same block limit
    many = TemplatedVocabulary().score_many(q, vecs)
    assert np.array_equal(bits(many), bits(full[2]))
    assert np.array_equal(bits(many), bits(KO.query_arrays(vecs, q)[2]))


@pytest.mark.parametrize("nq", [300, 5000])
def test_stored_lengths_around_the_pass(nq):
    q, vecs = BC.pass_world(nq, seed=nq)
    assert_same(database_of(vecs).query(q), KO.query_arrays(vecs, q), f"query {nq}")


def test_single_shared_word_at_every_chunk():
    q, vecs = BC.single_shared_world()
    got = database_of(vecs).query(q)
    want = KO.query_arrays(vecs, q)
    assert got[0].tolist() == [1] * len(vecs)
    assert got[1].tolist() == [1000 * p for p in BC.SINGLE_POSITIONS]
    assert_same(got, want, "one shared word")
    for p, v, s in zip(BC.SINGLE_POSITIONS, vecs, got[2].tolist()):
        vi, wi = q[1000 * p], v[1000 * p]
        assert bits(s) == bits(-((abs(vi - wi) - abs(vi)) - abs(wi)) / 2.0), p


@pytest.mark.parametrize("nq", BC.EDGE_QUERY_LENGTHS)
def test_query_lengths_at_the_lds_limit(nq):
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    q, vecs = BC.extended_world(nq, seed=nq)
    assert len(q) == nq
    want = KO.query_arrays(vecs, q)
    assert_same(database_of(vecs, 128, 1 << 15).query(q), want, f"query {nq}")
    assert np.array_equal(bits(TemplatedVocabulary().score_many(q, vecs)), bits(want[2]))


def test_weights_outside_the_unit_interval():
    """Zero, subnormal, huge and negative weights: the oracle is Python double arithmetic, subnormals kept."""
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    q, vecs = BC.odd_weight_world()
    want = KO.query_arrays(vecs, q)
    assert_same(database_of(vecs).query(q), want, "odd weights")
    assert np.array_equal(bits(TemplatedVocabulary().score_many(q, vecs)), bits(want[2]))


# ---- 5. shared objects under threads ------------------------------------------------------------------------------
def test_vocabulary_and_database_shared_by_threads(ragged):
    """Tracking, LocalMapping and LoopClosing share one vocabulary and one keyframe database (System.py:38-64):
    four threads descend 1..600 descriptors and query at sizes drawn per iteration (so the scratch buffers are
    re-allocated under the other threads) while one of them adds and erases; every result against an oracle
    result computed before the threads start."""
    t, o, _ = ragged
    v = native_of(t)
    pool = VS.query_descriptors(t, 91, 600)
    want_desc = [o.descend(x, 2) for x in pool]
    r = np.random.default_rng(92)
    base = BC.random_vec(r, 400)
    stored = [BC.overlapping_vec(r, base, int(r.integers(0, 300))) for _ in range(300)]
    queries = [BC.overlapping_vec(r, base, n, 0.9) for n in (1, 40, 200, 399)]
    want_q = [KO.query_arrays(stored, q) for q in queries]
    extra = [BC.overlapping_vec(r, base, 1500) for _ in range(30)]
    db = database_of(stored, 4, 64)   # small hints: the writer's 45 000 words make the arena regrow under the readers
    regrows = db.stats()["regrows"]
    errors = []

    def work(seed):
        rng = np.random.default_rng(seed)
        try:
            for it in range(30):
                n, a = int(rng.integers(1, 601)), int(rng.integers(0, 600))
                idx = (a + np.arange(n)) % 600
                word, node, w = v.descend(pool[idx], 2)
                if list(zip(word.tolist(), node.tolist(), w.tolist())) != [want_desc[i] for i in idx.tolist()]:
                    errors.append(("descend", seed, it, n))
                if seed == 0:
                    slot = db.add(extra[it])
                    if slot < 300:
                        errors.append(("slot", seed, it, slot))
                    if it % 2:
                        db.erase(slot)
                k = int(rng.integers(0, len(queries)))
                got = db.query(queries[k])
                if len(got[0]) < 300:
                    errors.append(("short", seed, it, len(got[0])))
                    continue
                for g, x, name in zip(got, want_q[k], ("common", "first", "score")):
                    g, x = (bits(g[:300]), bits(x)) if name == "score" else (g[:300], x)
                    if not np.array_equal(g, x):
                        errors.append((name, seed, it, k))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(("raised", seed, repr(e)))

    ths = [threading.Thread(target=work, args=(s,)) for s in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors[:5]
    st = db.stats()
    assert st["n_slots"] == 330 and st["n_live"] == 315 and st["regrows"] > regrows
