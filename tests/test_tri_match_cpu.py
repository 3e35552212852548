"""The triangulation match without a GPU: the array oracle against goldens made by the reference itself
(tests/golden/gen_golden_tri_match.py and the tri0_* / tri1_* entries of matcher_kf_*.npz), the claims of the crafted
cases, the keyframe packer, the new symbols, and every argument check of orbfe_tri_match, all of which come before
any device call."""
import ctypes as C
import re

import numpy as np
import pytest

import matcher_world as MW
import tri_match_cases as TC
import tri_match_oracle as O
from conftest import GOLDEN, ROOT

NEW = ("orbfe_tri_match", "orbfe_tri_match_last_ms")


class Z:
    def __init__(self, d):
        self._d, self.files = d, list(d.keys())

    def __getitem__(self, k):
        return self._d[k]


def golden_world():
    """(z, [(j, F12, [(only_stereo, check_ori, stop, pairs)])]) of tests/golden/tri_match.npz."""
    g = np.load(GOLDEN / "tri_match.npz", allow_pickle=False)
    z = TC.decode_world(g)
    runs = []
    for j in range(1, int(g["n_kf"])):
        runs.append((j, g[f"F12_{j}"], [(bool(only), bool(ori), int(g[f"r{c}_{j}_stop"]), g[f"r{c}_{j}_pairs"])
                                        for c, (only, ori) in enumerate(zip(g["only_stereo"], g["check_ori"]))]))
    return z, runs


def test_oracle_reproduces_the_reference():
    z, runs = golden_world()
    frames = [TC.world_frame(z, j) for j in range(int(z["n_kf"]))]
    assert len(runs) == 8 and len(frames[0]["desc"]) == 300
    assert int((frames[0]["flags"] & O.ELIGIBLE).sum()) > 200  # most of keyframe 0 holds no map point
    dropped = by_epi = 0
    for j, F12, lst in runs:
        e = TC.world_epipole(z["kf0_T"], z[f"kf{j}_T"])
        for only, ori, stop, pairs in lst:
            raw = O.match_pair(frames[0], frames[j], F12, e[0], e[1], 50, only)
            assert raw[5] == stop == 0 and raw[4] == 0
            assert not ori or O.cut_is_stable(raw[2])
            got = O.finish(raw[0], raw[1], raw[2], ori)
            assert got == [tuple(p) for p in pairs.tolist()], (j, only, ori)
            assert len(got) > 0
            dropped += int(raw[3]) - len(got)
            if not ori:
                free = O.match_pair(frames[0], frames[j], F12, e[0], e[1], 50, only, use_epi=False)
                by_epi += int((free[0] != raw[0]).sum())
    assert dropped > 10 and by_epi > 10  # a working rotation cut, a line test that decides


@pytest.mark.parametrize("case", range(7))
def test_oracle_reproduces_the_keyframe_goldens(case):
    """tri0_* / tri1_* of matcher_kf_<case>.npz, including the two searches out of which StopIteration escaped."""
    g = np.load(GOLDEN / f"matcher_kf_{case}.npz", allow_pickle=False)
    f1, f2 = TC.world_frame(g, 0), TC.world_frame(g, 1)
    e = TC.world_epipole(g["kf0_T"], g["kf1_T"])
    ori = case != 3
    for only in (False, True):
        key = f"tri{int(only)}"
        raw = O.match_pair(f1, f2, g[f"{key}_F12"], e[0], e[1], 50, only)
        assert raw[5] == int(g[f"{key}_stop"]) == int(case == 5)
        if raw[5]:
            assert raw[3] == 0 and bool((raw[0] == -1).all())
            continue
        assert raw[4] == 0 and (not ori or O.cut_is_stable(raw[2]))
        assert O.finish(raw[0], raw[1], raw[2], ori) == [tuple(p) for p in g[f"{key}_pairs"].tolist()]


CASES = TC.all_cases()
ORACLE = {c["name"]: TC.oracle(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_holds_its_claim(case):
    res = ORACLE[case["name"]]
    case["check"](res)
    assert (sum(r[3] for r in res) == 0) == case["empty"]
    if case["name"] != "marginal":
        assert all(r[4] == 0 for r in res)
    for r, (a, _) in zip(res, case["pairs"]):
        assert len(r[0]) == len(case["frames"][a]["desc"]) and int((r[0] >= 0).sum()) == r[3] == int(r[2].sum())


def test_the_set_is_not_vacuous():
    """Over the whole set a winner differs from what the search would take without the epipole gate, without the
    line test, and without blocking."""
    diff = {"use_ex": 0, "use_epi": 0, "block": 0}
    for c in CASES:
        for k in diff:
            for r, w in zip(TC.oracle(c, **{k: False}), ORACLE[c["name"]]):
                diff[k] += int(((r[0] != w[0]) & (w[0] >= 0)).sum())
    assert all(v > 0 for v in diff.values()), diff
    lens = {len(O.runs(c["frames"][b])[7]) for c in CASES if c["name"].startswith("run2_") for _, b in c["pairs"]}
    assert lens == {1, 63, 64, 65, 129}


def test_walk_is_the_references_not_a_merge():
    from pyorbslam_amd.matcher import ORBMatcher
    rng = np.random.Generator(np.random.PCG64(3))
    stops = 0
    for _ in range(200):
        n1 = sorted(set(rng.integers(0, 12, int(rng.integers(0, 9))).tolist()))
        n2 = sorted(set(rng.integers(0, 12, int(rng.integers(0, 9))).tolist()))
        vis, stopped = O.walk(n1, n2)
        fv1, fv2 = {k: [("a", k)] for k in n1}, {k: [("b", k)] for k in n2}
        try:
            want = ORBMatcher._triangulation_nodes(fv1, fv2)
            assert not stopped and [(fv1[n1[a]], fv2[n2[b]]) for a, b in vis] == want
        except StopIteration:
            assert stopped and vis == []
            stops += 1
    assert 10 < stops < 190


# ---- the packer -------------------------------------------------------------------------------------------------

def test_packer_round_trips():
    from pyorbslam_amd import matcher
    z, _ = golden_world()
    w = TC.build_world(z)
    for j in (0, 3):
        t, f = matcher._tri_frame(w.kfs[j]), TC.world_frame(z, j)
        for k in ("desc", "angle", "xy", "octave", "flags", "fv_node", "fv_end", "fv_idx", "thr_epi", "thr_ex"):
            got = getattr(t, k)
            assert got.dtype == f[k].dtype and np.array_equal(got, f[k]), (j, k)
        assert t.xy_f32
    kf = w.kfs[1]
    assert matcher._tri_frame(kf) is not None
    keep = kf.mvKeysUn[4].pt
    kf.mvKeysUn[4].pt = (np.float32(keep[0]), keep[1])      # a coordinate that is not a double
    assert matcher._tri_frame(kf) is None
    kf.mvKeysUn[4].pt = keep
    kf.mvKeysUn[4].octave = 8                                # outside the level tables
    assert matcher._tri_frame(kf) is None
    kf.mvKeysUn[4].octave = -1                               # Python would index from the end
    assert matcher._tri_frame(kf) is None
    kf.mvKeysUn[4].octave = 0
    fv = kf.mFeatVec
    kf.mFeatVec = dict(reversed(list(fv.items())))           # keys not ascending
    assert matcher._tri_frame(kf) is None
    kf.mFeatVec = fv
    kf.mvLevelSigma2 = [float("inf")] * 8
    assert matcher._tri_frame(kf) is None
    kf.mvLevelSigma2 = list(MW.SIG2)
    assert matcher._tri_frame(kf) is not None
    # the epipole: doubles as they are, a float32 one unless a mono feature lies on its threshold
    f2 = matcher._tri_frame(kf)
    assert matcher._tri_epipole(1.5, np.float64(2.5), f2) == (1.5, 2.5)
    assert matcher._tri_epipole(np.array([1.5], np.float32), np.array([2.5], np.float32), f2) == (1.5, 2.5)
    assert matcher._tri_epipole(1, 2.5, f2) is None and matcher._tri_epipole(float("nan"), 2.5, f2) is None
    i = int(np.flatnonzero(((f2.flags & 2) == 0) & (f2.octave == 0))[0])  # mono, thr_ex = 100: ten pixels away
    x, y = float(f2.xy[i, 0]), float(f2.xy[i, 1])
    assert matcher._tri_epipole(np.float32(x + 10.0), np.float32(y), f2) is None
    assert matcher._tri_epipole(np.float32(x + 10.5), np.float32(y), f2) is not None
    assert matcher._tri_epipole(x + 10.0, y, f2) == (x + 10.0, y)


def test_many_fall_back_without_a_launch(monkeypatch):
    """F12 as float32, and a keyframe the packer refuses: every element takes the single search, nothing is launched."""
    from pyorbslam_amd import matcher
    from test_matcher_kf import _cpu_batched
    monkeypatch.setattr(matcher.ORBMatcher, "_batched", staticmethod(_cpu_batched))
    monkeypatch.setattr(matcher, "tri_match_arrays", lambda *a, **k: pytest.fail("launched"))
    z, runs = golden_world()
    w = TC.build_world(z)
    m = matcher.ORBMatcher(0.6, True)
    F = [runs[0][1].astype(np.float32), runs[1][1].astype(np.float32)]
    want = [m.search_for_triangulation(w.kfs[0], kf, f) for kf, f in zip(w.kfs[1:3], F)]
    assert m.search_for_triangulation_many(w.kfs[0], w.kfs[1:3], F) == want and len(want[0]) > 0
    w.kfs[0].mvKeysUn[0].angle = 0.1  # a double that is no float32 value
    w.kfs[0].mvKeysUn = list(w.kfs[0].mvKeysUn)
    F = [runs[0][1], runs[1][1]]
    want = [m.search_for_triangulation(w.kfs[0], kf, f, True) for kf, f in zip(w.kfs[1:3], F)]
    assert m.search_for_triangulation_many(w.kfs[0], w.kfs[1:3], F, True) == want
    assert m.search_for_triangulation_many(w.kfs[0], [], []) == []


# ---- the ABI ----------------------------------------------------------------------------------------------------

def test_new_symbols_resolve_and_abi_is_still_9():
    from pyorbslam_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.orbfe_abi_version() == 9 == _lib.ORBFE_ABI_VERSION
    assert C.sizeof(_lib.TriMatchOut) == 6 * C.sizeof(C.c_void_p)


def test_table_and_header_agree():
    from pyorbslam_amd import _lib
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_tri_match_out \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in _lib.TriMatchOut._fields_]
    for k in ("ELIGIBLE", "STEREO", "MARGINAL"):
        assert int(re.search(rf"#define ORBFE_TRI_{k} (\d+)", hdr).group(1)) == getattr(_lib, f"ORBFE_TRI_{k}")
    assert (O.ELIGIBLE, O.STEREO) == (_lib.ORBFE_TRI_ELIGIBLE, _lib.ORBFE_TRI_STEREO)
    assert O.MARGINAL == _lib.ORBFE_TRI_MARGINAL
    assert int(re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1)) == 9


ARRAYS = ("desc", "angle", "xy", "octave", "flags", "off", "fv_off", "fv_node", "fv_end", "fv_idx", "lvl_off",
          "thr_epi", "thr_ex")
OUTS = ("match12", "bin12", "hist", "n_raw", "status", "stopped")


class HostCall:
    """orbfe_tri_match over a small valid input; each test breaks one thing."""

    def __init__(self):
        f1, f2 = TC.FrameBuilder(), TC.FrameBuilder()
        for k in (1, 1, 4, 9):
            f1.add(k, TC.D(k))
            f2.add(k, TC.D(k, 100))
        self.a = TC.pack([f1.build(), f2.build()])
        self.pairs = np.array([[0, 1], [1, 1]], np.int32)
        self.F12 = np.stack([TC.F_ROW, TC.F_ROW])
        self.epi = np.array([TC.FAR, TC.FAR], np.float64)
        self.stride, self.th = 4, 50
        self.o = dict(match12=np.full((2, 4), -7, np.int32), bin12=np.full((2, 4), -7, np.int8),
                      hist=np.full((2, 32), -7, np.int32), n_raw=np.full(2, -7, np.int32),
                      status=np.full(2, -7, np.int32), stopped=np.full(2, -7, np.int32))
        self.null = set()

    def run(self, n_frames=2, n_pairs=2):
        from pyorbslam_amd import _lib
        p = lambda k, v: None if k in self.null else _lib.ptr(v)  # noqa: E731
        out = _lib.TriMatchOut(**{k: None if k in self.null else v.ctypes.data for k, v in self.o.items()})
        rc = _lib.lib().orbfe_tri_match(*[p(k, self.a[k]) for k in ARRAYS[:6]], n_frames,
                                        *[p(k, self.a[k]) for k in ARRAYS[6:]], p("pairs", self.pairs),
                                        p("F12", self.F12), p("epipole", self.epi), n_pairs, self.th, 0,
                                        None if "out" in self.null else C.byref(out), self.stride)
        return rc, _lib.lib().orbfe_last_error().decode()

    def untouched(self):
        return all(bool((x == -7).all()) for x in self.o.values())


def refused(h, *words):
    from pyorbslam_amd import _lib
    rc, msg = h.run()
    assert rc == _lib.ORBFE_EINVAL and all(w in msg for w in words), (rc, msg)
    assert "ORBFE_" not in msg and h.untouched()


def test_feature_vector_checks_are_those_of_the_bow_match():
    h = HostCall()
    h.a["fv_node"][:3] = [1, 1, 9]
    refused(h, "strictly ascending")
    h = HostCall()
    h.a["fv_end"][:3] = [2, 1, 4]
    refused(h, "must not decrease")
    h = HostCall()
    h.a["fv_end"][:3] = [2, 3, 5]
    refused(h, "past the index count")
    for v in (4, -1):
        h = HostCall()
        h.a["fv_idx"][5] = v
        refused(h, "out of range")
    h = HostCall()
    h.a["fv_idx"][1] = h.a["fv_idx"][0]
    refused(h, "appears twice")
    for v in (2, -1):
        h = HostCall()
        h.pairs[1, 0] = v
        refused(h, "does not exist")


def test_frame_above_the_cap_offsets_and_stride():
    from pyorbslam_amd import _lib
    h = HostCall()
    h.a["off"] = np.array([0, _lib.ORBFE_BOW_MAX_FRAME + 1, _lib.ORBFE_BOW_MAX_FRAME + 5], np.int64)
    refused(h, f"limit of {_lib.ORBFE_BOW_MAX_FRAME} per frame")
    for k in ("off", "fv_off", "lvl_off"):
        h = HostCall()
        h.a[k][0] = 1
        refused(h, "must be 0")
    h = HostCall()
    h.a["lvl_off"][1:] = [3, 2]
    refused(h, "must not decrease")
    h = HostCall()
    h.stride = 3
    refused(h, "out_stride")
    for th in (-1, 257):
        h = HostCall()
        h.th = th
        refused(h, "bad argument")


def test_octaves_and_finiteness_name_the_frame_or_pair():
    h = HostCall()
    h.a["octave"][5] = 3
    refused(h, "frame 1", "octave")
    h = HostCall()
    h.a["octave"][0] = -1
    refused(h, "frame 0", "octave")
    for v in (np.nan, np.inf):
        h = HostCall()
        h.a["xy"][6, 1] = v
        refused(h, "frame 1", "coordinate", "finite")
        h = HostCall()
        h.a["thr_epi"][1] = v
        refused(h, "frame 0", "threshold", "finite")
        h = HostCall()
        h.a["thr_ex"][5] = -v
        refused(h, "frame 1", "threshold", "finite")
        h = HostCall()
        h.F12[1, 2, 2] = v
        refused(h, "pair 1", "F12", "finite")
        h = HostCall()
        h.epi[0, 1] = v
        refused(h, "pair 0", "epipole", "finite")


@pytest.mark.parametrize("name", ARRAYS + ("pairs", "F12", "epipole", "out") + OUTS)
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
    assert _lib.lib().orbfe_tri_match_last_ms(None) == _lib.ORBFE_EINVAL
