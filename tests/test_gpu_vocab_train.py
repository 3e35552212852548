"""orbfe_vocab_train on the device against the definition (tests/vocab_train_definition.py): every comparison is
exact — parent, is_leaf, desc, word_id, the weights as uint64 bits, and the stats counters."""
import ctypes as C

import numpy as np
import pytest

import vocab_train_cases as TC
import vocab_train_definition as VD
from pyorbslam_amd import _lib
from pyorbslam_amd.vocabulary import TemplatedVocabulary

pytestmark = pytest.mark.gpu

W_NAME = {v: k for k, v in VD.WEIGHTINGS.items()}
COUNTERS = ("nodes_split", "iter_sum", "iter_max", "capped", "empty_dropped", "short_seeded")


def assert_same_tree(got: dict, want: dict):
    for key in ("parent", "is_leaf", "desc", "word_id"):
        assert got[key].shape == want[key].shape, key
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["weight"].view(np.uint64), want["weight"].view(np.uint64))


def assert_same_stats(got: dict, want: dict):
    for key in ("n_desc", "n_nodes", "n_words"):
        assert got[key] == want[key], key
    for key in COUNTERS:
        assert got[key] == want[key], key


def train(c) -> TemplatedVocabulary:
    voc = TemplatedVocabulary(c["k"], c["L"], W_NAME[c["weighting"]], "L1_NORM")
    assert voc.create(c["frames"], seed=c["seed"], max_iter=c["max_iter"]) is voc
    return voc


def check(c, want):
    voc = train(c)
    assert_same_tree(voc.node_arrays(), want)
    assert_same_stats(voc.train_stats(), want["stats"])
    info = voc.info()
    assert (info.k, info.L, info.weighting, info.scoring) == (c["k"], c["L"], c["weighting"], 0)
    assert voc.size() == want["stats"]["n_words"]
    return voc


@pytest.mark.parametrize("name", list(TC.CASES))
def test_case_equals_definition(name):
    check(TC.CASES[name], TC.expected(name))


@pytest.fixture(scope="module")
def medium():
    c = TC.medium()
    return c, VD.train(c["frames"], c["k"], c["L"], c["weighting"], c["seed"], c["max_iter"])


def test_medium_equals_definition(medium):
    c, want = medium
    voc = check(c, want)
    st = voc.train_stats()
    assert max(st["iter_max"]) <= 31 and sum(st["capped"]) == 0
    assert st["kernel_ms"] > 0 and abs(sum(st["depth_ms"]) + st["weight_ms"] - st["kernel_ms"]) < 1e-6


def test_bare_root_from_empty_images():
    voc = TemplatedVocabulary(3, 2).create([np.zeros((0, 32), np.uint8)] * 2)
    a = voc.node_arrays()
    assert len(a["parent"]) == 1 and voc.size() == 0 and voc.train_stats()["n_nodes"] == 1


def test_same_descriptors_cut_two_ways():
    a, b = TC.expected("frames_cut_a"), TC.expected("frames_cut_b")
    for key in ("parent", "is_leaf", "desc", "word_id"):
        assert np.array_equal(a[key], b[key])
    assert not np.array_equal(a["weight"], b["weight"])
    ga, gb = train(TC.CASES["frames_cut_a"]).node_arrays(), train(TC.CASES["frames_cut_b"]).node_arrays()
    assert_same_tree(ga, a)
    assert_same_tree(gb, b)


def raw_train(desc_ptr, on_device, start, count, c):
    prm = _lib.VocabTrainParams(c["k"], c["L"], c["weighting"], 0, c["max_iter"], 0, c["seed"])
    h, st = C.c_void_p(), _lib.VocabTrainStats()
    _lib.call("orbfe_vocab_train", C.c_void_p(desc_ptr), on_device, _lib.ptr(start), _lib.ptr(count), len(count),
              C.byref(prm), C.byref(h), C.byref(st))
    voc = TemplatedVocabulary(c["k"], c["L"])
    voc._replace(h)
    return voc


def test_host_and_device_pointers_and_a_strided_layout_with_gaps():
    import torch
    name = "node_257"
    c, want = TC.CASES[name], TC.expected(name)
    count = np.array([len(f) for f in c["frames"]], np.int32)
    # image f at a stride of its own with junk between the images, the images not in address order
    slot = int(count.max()) + 5
    where = np.array([2, 0, 1], np.int64)[:len(count)]
    buf = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (slot * 4, 32), dtype=np.uint8)
    start = where * slot + 3
    for f, fr in enumerate(c["frames"]):
        buf[start[f]:start[f] + len(fr)] = fr
    host = raw_train(buf.ctypes.data, 0, start, count, c)
    dev_buf = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    dev = raw_train(dev_buf.data_ptr(), 1, start, count, c)
    assert_same_tree(host.node_arrays(), want)
    assert_same_tree(dev.node_arrays(), want)


def test_saved_and_loaded_tree_descends_the_training_set_to_the_same_words(tmp_path):
    c = TC.CASES["many_small"]
    voc = train(c)
    path = tmp_path / "trained.txt"
    voc.save_to_text_file(path)
    back = TemplatedVocabulary()
    assert back.load_from_text_file(path)
    assert_same_tree(back.node_arrays(), voc.node_arrays())
    D = np.concatenate(c["frames"])
    w0, n0, x0 = voc.descend(D, 1)
    w1, n1, x1 = back.descend(D, 1)
    assert np.array_equal(w0, w1) and np.array_equal(n0, n1) and np.array_equal(x0.view(np.uint64), x1.view(np.uint64))
    want = TC.expected("many_small")
    assert np.array_equal(w0, want["word_id"][VD.descend(want, D)])


def test_front_end_trains_on_its_resident_descriptors():
    import torch
    from pyorbslam_amd import synth
    from pyorbslam_amd.batch import StereoFrontEnd
    w, h, pairs = 211, 157, 3
    fe = StereoFrontEnd(w, h, max_pairs=pairs, nfeatures=500)
    imgs = np.stack([im for p in range(pairs) for im in synth.make_pair(20 + p, w, h)])
    fe.enqueue(torch.from_numpy(imgs).cuda(), pairs)
    for side, step in (("left", 2), ("both", 1)):
        trained = fe.train_vocabulary(k=4, L=3, side=side, seed=5)
        frames = [fe.fetch_image(i)[1] for i in range(0, 2 * pairs, step)]
        assert sum(len(f) for f in frames) > 100
        same = TemplatedVocabulary(4, 3).create(frames, seed=5)
        assert_same_tree(trained.node_arrays(), same.node_arrays())
        assert trained.train_stats()["n_desc"] == sum(len(f) for f in frames)
        assert fe.bow(trained, levels_up=1, side=side) == len(frames)
        for i, f in enumerate(frames):
            got, want = fe.fetch_bow(i), trained.bow_many([f], levels_up=1)[0]
            assert got.n_kept == want.n_kept
            for a, b in zip(got[:5], want[:5]):
                assert np.array_equal(a, b)
            assert got.dicts() == tuple(trained.transform(f, levels_up=1))
