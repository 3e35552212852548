"""Vocabulary training without a device: the definition against the reference's FORB goldens, what each named case
reaches, the text writer, and every refusal of orbfe_vocab_train (all made before the first device call)."""
import ctypes as C
import re

import numpy as np
import pytest

import vocab_synth as VS
import vocab_train_cases as TC
import vocab_train_definition as VD
from conftest import GOLDEN, ROOT
from oracle.vocab_oracle import VocabOracle
from pyorbslam_amd import _lib
from pyorbslam_amd.vocabulary import TemplatedVocabulary

NEW = ["orbfe_vocab_train", "orbfe_vocab_save_text"]
GROUPS = (1, 2, 3, 4, 5, 8, 9)
GOLDEN_TREES = {"k3L3": (3, 3, (1, 2)), "k5L2_dup": (5, 2, (0, 1))}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "vocab_train_ref.npz", allow_pickle=False)


# ---- the definition's pieces against the reference's -------------------------------------------------------------

def test_mean_and_distance_equal_the_reference(gold):
    halves = 0
    for n in GROUPS:
        g = gold[f"mean_in_{n}"]
        assert len(g) == n
        assert np.array_equal(VD.mean_value(g), gold[f"mean_out_{n}"]), n
        halves += int((np.unpackbits(g, axis=1).sum(axis=0) * 2 == n).sum())
    assert halves >= 4 * 128  # the even groups have exact-half counts in half of their bits
    for (a, b), want in zip(gold["dist_in"], gold["dist_out"].tolist()):
        assert VD.distance(a, b) == want
    assert gold["dist_out"][0] == 0 and gold["dist_out"][1] == 256


def test_splitmix_draws():
    # splitmix64's published first outputs for the state 0: the state advances by the golden ratio constant
    assert VD.draw(0, 0, 0) == 0xE220A8397B1DCDAF
    assert VD.draw(0, 0, 1) == 0x6E789E6AA1B965F4
    assert VD.draw(5, 3, 2) == VD.splitmix64(5 + 99 * 0x9E3779B97F4A7C15)


# ---- each case reaches what it aims at ---------------------------------------------------------------------------

def stats(name):
    return TC.expected(name)["stats"]


def test_cases_reach_what_they_aim_at():
    assert sum(stats("emptied_cluster")["empty_dropped"]) > 0
    assert sum(stats("node_2048")["empty_dropped"]) > 0
    assert stats("three_values_of_50")["short_seeded"][0] == 1 and stats("three_values_of_50")["n_nodes"] == 7
    assert stats("identical")["short_seeded"][:4] == [1, 1, 1, 1]
    for name, it in (("capped_2", 2), ("capped_3", 3), ("seeds_only", 1)):
        assert sum(stats(name)["capped"]) > 0 and max(stats(name)["iter_max"]) == it
    assert sum(stats("k20_L1")["ties"]) > 0 and sum(stats("many_small")["ties"]) > 0
    assert sum(stats("node_65")["exact_half"]) > 0 and sum(stats("k20_L1")["exact_half"]) > 0
    assert stats("L10_on_40")["single_above_L"] > 0 and stats("many_small")["single_above_L"] > 0


def test_shapes_of_the_cases():
    for name, n in (("n1", 1), ("n2", 2), ("n_k", 4), ("n_k_plus_1", 5)):
        assert stats(name)["n_desc"] == n and TC.CASES[name]["k"] == 4
    assert stats("n_k")["iter_sum"][0] == 0 and stats("n_k_plus_1")["iter_sum"][0] > 0
    t = TC.expected("identical")  # a chain of single children down to depth L
    assert t["parent"].tolist() == [0, 0, 1, 2, 3] and t["members"].tolist() == [30] * 5
    for n in TC.EDGE_SIZES:
        assert stats(f"node_{n}")["n_desc"] == n
    assert {TC.WAVE + d for d in (-1, 0, 1)} | {TC.CHUNK + d for d in (-1, 0, 1)} <= set(TC.EDGE_SIZES)
    t = TC.expected("many_small")
    at2 = t["members"][(t["depth_of"] == 2) & (t["members"] > 1)]
    assert len(at2) >= 250 and np.median(at2) <= 30 and stats("many_small")["nodes_split"][2] == len(at2)
    t = TC.expected("big_beside_tiny")
    at1 = t["members"][t["depth_of"] == 1]
    assert at1.max() > 2 * TC.CHUNK and (at1 <= 30).sum() >= 2 and stats("big_beside_tiny")["nodes_split"][1] == 4
    assert stats("k20_L1")["n_words"] == 20 and TC.CASES["k20_L1"]["k"] == 20
    assert len(np.concatenate(TC.CASES["L10_on_40"]["frames"])) == 40 and TC.expected("L10_on_40")["depth_of"].max() > 5


def test_seed_draws_of_the_one_iteration_cases():
    tr = []
    TC.expected("seeds_only", trace=tr)
    assert any(x["exact"] for x in tr) and any(x["pick"] == 0 for x in tr) and any(x["pick"] == x["n"] - 1 for x in tr)
    for name, pick in (("cut_is_S_last", 11), ("cut_is_S_first", 0)):
        tr = []
        t = TC.expected(name, trace=tr)
        assert len(tr) == 1 and tr[0]["S"] == 1 == tr[0]["cut"] and tr[0]["pick"] == pick and tr[0]["exact"]
        # max_iter = 1: the centres are the picks
        D = np.concatenate(TC.CASES[name]["frames"])
        assert {bytes(d) for d in t["desc"][1:]} == {bytes(d) for d in D}


def test_weights_of_the_cases():
    w = {name: TC.expected(f"weights_{name}")["weight"] for name in VD.WEIGHTINGS}
    assert np.array_equal(w["TF_IDF"], w["IDF"]) and np.array_equal(w["TF"], w["BINARY"])
    assert w["TF"].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0] and np.all(w["IDF"][1:] > 0)
    assert any(len(f) == 0 for f in TC.CASES["weights_IDF"]["frames"])
    z = TC.expected("weight_zero")
    assert (z["weight"][1:] == 0.0).sum() >= 1 and (z["weight"][1:] > 0).sum() >= 1
    a, b = TC.expected("frames_cut_a"), TC.expected("frames_cut_b")
    assert np.array_equal(a["desc"], b["desc"]) and not np.array_equal(a["weight"], b["weight"])


# ---- the text writer ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(seed=2, k=4, L=3, p_stop=0.2, p_zero=0.2), dict(seed=3, k=10, L=2, order="dfs")])
def test_save_and_load_return_identical_node_arrays(kw, tmp_path):
    t = VS.make_tree(**kw)
    t["weight"][1:6] = [1e-05, 2.4849066497880004, 1.0, 5e-324, 1.7976931348623157e308]
    v = TemplatedVocabulary(t["k"], t["L"]).from_arrays(t["parent"], t["is_leaf"], t["desc"], t["weight"])
    path, ref_path = tmp_path / "saved.txt", tmp_path / "repr.txt"
    v.save_to_text_file(path)
    VS.write_text(t, ref_path)
    assert path.read_text() == ref_path.read_text()  # the shortest round-trip decimals, as repr writes them
    back = TemplatedVocabulary()
    assert back.load_from_text_file(path)
    a, b = v.node_arrays(), back.node_arrays()
    for key in ("parent", "is_leaf", "desc", "word_id"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["weight"].view(np.uint64), b["weight"].view(np.uint64))
    assert np.array_equal(a["weight"].view(np.uint64), t["weight"].view(np.uint64))


def test_save_refusals(tmp_path):
    L = _lib.lib()
    v = TemplatedVocabulary(3, 2)
    assert L.orbfe_vocab_save_text(None, str(tmp_path / "x.txt").encode()) == _lib.ORBFE_EINVAL
    assert L.orbfe_vocab_save_text(v._handle(), None) == _lib.ORBFE_EINVAL
    assert L.orbfe_vocab_save_text(v._handle(), str(tmp_path / "no" / "dir.txt").encode()) == _lib.ORBFE_EINVAL
    v.save_to_text_file(tmp_path / "root.txt")  # the bare root: the header alone
    assert (tmp_path / "root.txt").read_text() == "3 2 0 0\n"


@pytest.mark.parametrize("name", list(GOLDEN_TREES))
def test_golden_trees_give_the_reference_transforms(name, gold, tmp_path):
    k, L, lups = GOLDEN_TREES[name]
    path = tmp_path / "voc.txt"
    path.write_bytes(gold[f"{name}_text"].tobytes())
    v = TemplatedVocabulary()
    assert v.load_from_text_file(path) and (v.k, v.L) == (k, L)
    assert v.size() == int(gold[f"{name}_size"])
    a = v.node_arrays()
    o = VocabOracle(a["parent"], a["is_leaf"], a["desc"], a["weight"], L)
    for lu in lups:
        bv, fv = o.transform(gold[f"{name}_queries"], lu)
        assert list(bv.items()) == list(zip(gold[f"{name}_bv_word_{lu}"].tolist(), gold[f"{name}_bv_w_{lu}"].tolist()))
        idx = gold[f"{name}_fv_idx_{lu}"].tolist()
        off = np.concatenate([[0], np.cumsum(gold[f"{name}_fv_len_{lu}"])]).tolist()
        want = [(n, idx[off[j]:off[j + 1]]) for j, n in enumerate(gold[f"{name}_fv_node_{lu}"].tolist())]
        assert list(fv.items()) == want
    # the file is what save_to_text_file writes for the tree the definition trains
    v.save_to_text_file(tmp_path / "again.txt")
    assert (tmp_path / "again.txt").read_bytes() == path.read_bytes()


# ---- the ABI ------------------------------------------------------------------------------------------------------

def test_new_symbols_resolve_and_abi_is_still_9():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.orbfe_abi_version() == 9 == _lib.ORBFE_ABI_VERSION
    assert C.sizeof(_lib.VocabTrainParams) == 32
    assert C.sizeof(_lib.VocabTrainStats) == 8 * (3 + 7 * _lib.ORBFE_VOCAB_TRAIN_MAX_L + 2)


def test_table_and_header_agree():
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_vocab_train_params \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in _lib.VocabTrainParams._fields_]
    fields = re.search(r"typedef struct orbfe_vocab_train_stats \{(.*?)\}", code, flags=re.S).group(1)
    names = [n for decl in re.findall(r"(?:int64_t|double) ([^;]+);", fields) for n in re.findall(r"(\w+)(?:\[\w+\])?", decl)
             if not n.startswith("ORBFE")]
    assert names == [f[0] for f in _lib.VocabTrainStats._fields_]
    assert int(re.search(r"#define ORBFE_VOCAB_TRAIN_MAX_L (\d+)", hdr).group(1)) == _lib.ORBFE_VOCAB_TRAIN_MAX_L
    src = (ROOT / "pyorbslam_amd" / "csrc" / "orbfe_vocabtrain.hip").read_text()
    assert "pyorbslam_amd/csrc/orbfe_vocabtrain.hip" in (ROOT / "Makefile").read_text()
    for key, want in (("kTrainThreads", TC.THREADS), ("kTrainChunk", TC.CHUNK)):
        assert int(re.search(rf"constexpr int {key} = (\d+);", src).group(1)) == want


# ---- refusals, before any device call -----------------------------------------------------------------------------

class Call:
    """orbfe_vocab_train over a small valid input; each test breaks one thing."""

    def __init__(self):
        self.desc = np.zeros((6, 32), np.uint8)
        self.start = np.array([0, 2], np.int64)
        self.count = np.array([2, 4], np.int32)
        self.n_frames = 2
        self.prm = dict(k=3, L=2, weighting=0, scoring=0, max_iter=8, reserved=0, seed=1)
        self.null = set()

    def run(self):
        prm = _lib.VocabTrainParams(**self.prm)
        h, st = C.c_void_p(), _lib.VocabTrainStats()

        def arg(name, value):
            return None if name in self.null else value
        return _lib.lib().orbfe_vocab_train(arg("desc", _lib.ptr(self.desc)), 0, arg("start", _lib.ptr(self.start)),
                                            arg("count", _lib.ptr(self.count)), self.n_frames,
                                            arg("params", C.byref(prm)), arg("out", C.byref(h)), C.byref(st))


@pytest.mark.parametrize("field,value", [("k", 1), ("k", 21), ("L", 0), ("L", 11), ("weighting", -1), ("weighting", 4),
                                         ("scoring", -1), ("scoring", 6), ("max_iter", 0), ("max_iter", -3)])
def test_parameters_out_of_range_are_refused(field, value):
    c = Call()
    c.prm[field] = value
    assert c.run() == _lib.ORBFE_EINVAL


@pytest.mark.parametrize("null", ["desc", "start", "count", "params", "out"])
def test_null_pointers_are_refused(null):
    c = Call()
    c.null.add(null)
    assert c.run() == _lib.ORBFE_EINVAL


def test_bad_frames_are_refused():
    for n in (0, -1):
        c = Call()
        c.n_frames = n
        assert c.run() == _lib.ORBFE_EINVAL
    c = Call()
    c.count[1] = -1
    assert c.run() == _lib.ORBFE_EINVAL
    c = Call()
    c.start[0] = -1
    assert c.run() == _lib.ORBFE_EINVAL
    c = Call()
    c.count[:] = [2 ** 30, 2 ** 30]  # 2^31 in total: one above the limit
    assert c.run() == _lib.ORBFE_EINVAL
    assert "2^31" in _lib.lib().orbfe_last_error().decode()


def test_unknown_weighting_string_raises_before_the_call():
    with pytest.raises(ValueError):
        TemplatedVocabulary(3, 2, weighting="TFIDF").create([np.zeros((4, 32), np.uint8)])
    with pytest.raises(RuntimeError):
        TemplatedVocabulary(3, 2).train_stats()
