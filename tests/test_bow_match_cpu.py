"""The BoW-guided match without a GPU: the array oracle against goldens made by the reference itself
(tests/golden/gen_golden_bow_match.py), the new symbols, and every argument check of orbfe_bow_match, all of
which come before any device call."""
import ctypes as C
import re

import numpy as np
import pytest

import bow_match_cases as BC
import bow_match_oracle as O
from conftest import GOLDEN, ROOT

NEW = ("orbfe_bow_match", "orbfe_bow_match_device", "orbfe_bow_match_last_ms")
KEYS = ("desc", "angle", "elig", "fv_node", "fv_end", "fv_idx")


def golden_scenes(kind):
    """[(f1, f2, [(nnratio, check_ori, n, match)])] of tests/golden/bow_match_<kind>.npz."""
    z = np.load(GOLDEN / f"bow_match_{kind}.npz", allow_pickle=False)
    out = []
    for s in range(int(z["n_scenes"])):
        f1, f2 = ({k: z[f"s{s}_{side}_{k}"] for k in KEYS} for side in ("f1", "f2"))
        runs = [(float(nn), bool(ori), int(z[f"s{s}_r{c}_n"]), z[f"s{s}_r{c}_match"])
                for c, (nn, ori) in enumerate(zip(z["nnratio"], z["check_ori"]))]
        out.append((f1, f2, runs))
    return out


def finish(kind, raw, ori):
    """(n, match) as the golden stores them from a pair's raw outputs: kf_kf's match12, kf_f's match21."""
    m12, m21, n = O.reject(*raw) if ori else (raw[0], raw[1], int(raw[4]))
    return n, (m12 if kind == "kf_kf" else m21)


@pytest.mark.parametrize("kind", ["kf_kf", "kf_f"])
def test_oracle_reproduces_the_reference(kind):
    scenes = golden_scenes(kind)
    assert len(scenes) >= 10
    sizes, dropped, none_or_bad = [], 0, 0
    for f1, f2, runs in scenes:
        sizes.append(len(f1["desc"]))
        none_or_bad += int((f1["elig"] == 0).sum())
        for nn, ori, n, match in runs:
            raw = O.match_pair(f1, f2, True, kind == "kf_kf", 50, kind == "kf_f", nn)
            if ori:
                assert O.cut_is_stable(raw[3])
                dropped += int(raw[4]) - n
            got_n, got = finish(kind, raw, ori)
            assert got_n == n and np.array_equal(got, match)
    assert max(sizes) >= 300 and none_or_bad > 50 and dropped > 10  # big frames, unusable slots, a working cut


def test_new_symbols_resolve_and_abi_is_still_9():
    from pyorbslam_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.orbfe_abi_version() == 9 == _lib.ORBFE_ABI_VERSION
    assert C.sizeof(_lib.BowMatchOut) == 6 * C.sizeof(C.c_void_p)


def test_table_and_header_agree():
    from pyorbslam_amd import _lib
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_bow_match_out \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in _lib.BowMatchOut._fields_]
    assert int(re.search(r"#define ORBFE_BOW_BAD_PAIR (\d+)", hdr).group(1)) == _lib.ORBFE_BOW_BAD_PAIR == 16
    assert int(re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1)) == 9


class HostCall:
    """orbfe_bow_match over a small valid input; each test breaks one thing."""

    def __init__(self):
        f1, f2 = BC.FrameBuilder(), BC.FrameBuilder()
        for k in (1, 1, 4, 9):
            f1.add(k, BC.D(k))
            f2.add(k, BC.D(k, 100))
        self.a = BC.pack([f1.build(), f2.build()])
        self.pairs = np.array([[0, 1], [1, 1]], np.int32)
        self.stride = 4
        self.m12 = np.full((2, 4), -7, np.int32)
        self.m21 = np.full((2, 4), -7, np.int32)
        self.b12 = np.full((2, 4), -7, np.int8)
        self.hist = np.full((2, 32), -7, np.int32)
        self.n_raw = np.full(2, -7, np.int32)
        self.null = set()

    def run(self, n_frames=2, n_pairs=2):
        from pyorbslam_amd import _lib
        p = lambda k, v: None if k in self.null else _lib.ptr(v)  # noqa: E731
        a = self.a
        out = _lib.BowMatchOut(match12=None if "match12" in self.null else self.m12.ctypes.data,
                               match21=None if "match21" in self.null else self.m21.ctypes.data,
                               bin12=None if "bin12" in self.null else self.b12.ctypes.data,
                               hist=None if "hist" in self.null else self.hist.ctypes.data,
                               n_raw=None if "n_raw" in self.null else self.n_raw.ctypes.data, status=None)
        rc = _lib.lib().orbfe_bow_match(p("desc", a["desc"]), p("angle", a["angle"]), p("elig", a["elig"]), None,
                                        p("off", a["off"]), n_frames, p("fv_off", a["fv_off"]),
                                        p("fv_node", a["fv_node"]), p("fv_end", a["fv_end"]), p("fv_idx", a["fv_idx"]),
                                        p("pairs", self.pairs), n_pairs, 50, 0, 1.0,
                                        None if "out" in self.null else C.byref(out), self.stride)
        return rc, _lib.lib().orbfe_last_error().decode()

    def untouched(self):
        return all(bool((x == -7).all()) for x in (self.m12, self.m21, self.b12, self.hist, self.n_raw))


def refused(h, word):
    from pyorbslam_amd import _lib
    rc, msg = h.run()
    assert rc == _lib.ORBFE_EINVAL and word in msg, (rc, msg)
    assert "ORBFE_" not in msg and h.untouched()


def test_nodes_must_ascend_strictly():
    for bad in ([1, 1, 9], [4, 1, 9]):
        h = HostCall()
        h.a["fv_node"][:3] = bad
        refused(h, "strictly ascending")


def test_run_ends_must_not_decrease_or_pass_the_frame():
    h = HostCall()
    h.a["fv_end"][:3] = [2, 1, 4]
    refused(h, "must not decrease")
    h = HostCall()
    h.a["fv_end"][:3] = [2, 3, 5]
    refused(h, "past the index count")


def test_feature_index_out_of_range_or_twice():
    for v in (4, -1):
        h = HostCall()
        h.a["fv_idx"][5] = v
        refused(h, "out of range")
    h = HostCall()
    h.a["fv_idx"][1] = h.a["fv_idx"][0]
    refused(h, "appears twice")


def test_pair_index_out_of_range():
    for v in (2, -1):
        h = HostCall()
        h.pairs[1, 0] = v
        refused(h, "does not exist")


def test_frame_above_the_cap():
    from pyorbslam_amd import _lib
    h = HostCall()
    h.a["off"] = np.array([0, _lib.ORBFE_BOW_MAX_FRAME + 1, _lib.ORBFE_BOW_MAX_FRAME + 5], np.int64)
    refused(h, f"limit of {_lib.ORBFE_BOW_MAX_FRAME} per frame")


def test_offsets_and_stride():
    h = HostCall()
    h.a["off"][0] = 1
    refused(h, "must be 0")
    h = HostCall()
    h.a["off"][1:] = [5, 3]
    refused(h, "must not decrease")
    h = HostCall()
    h.stride = 3
    refused(h, "out_stride")


@pytest.mark.parametrize("name", ["desc", "angle", "off", "fv_off", "fv_node", "fv_end", "fv_idx", "pairs", "out",
                                  "match12", "match21", "bin12", "hist", "n_raw"])
def test_required_pointers(name):
    h = HostCall()
    h.null.add(name)
    refused(h, "null argument")


def test_nothing_to_do_needs_no_device():
    from pyorbslam_amd import _lib
    h = HostCall()
    assert h.run(n_pairs=0)[0] == 0 and h.untouched()
    assert h.run(n_pairs=-1)[0] == _lib.ORBFE_EINVAL
    assert h.run(n_frames=-1)[0] == _lib.ORBFE_EINVAL
    L = _lib.lib()
    assert L.orbfe_bow_match_last_ms(None) == _lib.ORBFE_EINVAL
    out = _lib.BowMatchOut()
    bow = _lib.BowOut()
    # the device entry: zero pairs launch nothing; bad strides and NULL outputs are refused before any launch
    args = [None, 0, None, 1, 0, None, 1, None, 0, None, 0, C.byref(bow), 0, None]
    assert L.orbfe_bow_match_device(*args, 0, 50, 0, 1.0, C.byref(out), 0, None) == 0
    assert L.orbfe_bow_match_device(*args, 1, 50, 0, 1.0, C.byref(out), 0, None) == _lib.ORBFE_EINVAL
    args[3] = 0  # count_stride
    assert L.orbfe_bow_match_device(*args, 0, 50, 0, 1.0, C.byref(out), 0, None) == _lib.ORBFE_EINVAL


def test_many_fallback_conditions_need_no_device():
    """_bow_frame refuses what the arrays cannot express, so the _many methods take the single search there."""
    import matcher_world as MW
    from pyorbslam_amd import matcher
    rng = np.random.Generator(np.random.PCG64(5))
    z = MW.make_world(rng, n_kf=2, n=60, n_mp=40, n_words=8)

    class Z:
        files = list(z.keys())

        def __getitem__(self, k):
            return z[k]
    w = MW.build(Z())
    kf = w.kfs[0]
    vp = kf.get_map_point_matches()
    f = matcher._bow_frame(kf, kf.mvKeysUn, vp)
    assert f is not None and len(f.desc) == 60 and f.fv_end[-1] == 60 and int(f.elig.sum()) == sum(
        1 for p in vp if p and not p.is_bad())
    kf.mvKeysUn[3].angle = np.float32(kf.mvKeysUn[3].angle)
    kf.mvKeysUn = list(kf.mvKeysUn)  # a new list: the angle cache is keyed by it
    assert matcher._bow_frame(kf, kf.mvKeysUn, vp) is None
    kf = w.kfs[1]
    vp = kf.get_map_point_matches()
    assert matcher._bow_frame(kf, kf.mvKeysUn, vp) is not None
    keep = kf.mFeatVec
    kf.mFeatVec = dict(reversed(list(keep.items())))
    assert matcher._bow_frame(kf, kf.mvKeysUn, vp) is None      # keys not ascending
    kf.mFeatVec = {**keep, 10 ** 6: [0]}
    assert matcher._bow_frame(kf, kf.mvKeysUn, vp) is None      # an index in two runs
    kf.mFeatVec = {**keep, 10 ** 6: [60]}
    assert matcher._bow_frame(kf, kf.mvKeysUn, vp) is None      # an index outside the frame
    kf.mFeatVec = keep
    kf.mvKeysUn[0].angle = 0.1                                   # a double that is no float32 value
    kf.mvKeysUn = list(kf.mvKeysUn)
    assert matcher._bow_frame(kf, kf.mvKeysUn, vp) is None
