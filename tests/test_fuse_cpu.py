"""The many-keyframe fusion without a GPU: the array oracle and its replay against the golden made by the reference
itself (tests/golden/gen_golden_fuse.py), the soundness of the error bound (every item the oracle does not mark
decides as the reference's own expressions do) and the share of marked items, the claims of the crafted cases, the
keyframe packer, the new symbols, and every argument check of orbfe_fuse_search, all of which come before any device
call."""
import ctypes as C
import re

import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as O
import matcher_world as MW
from conftest import GOLDEN, ROOT
from pyorbslam_amd import _lib as LIB

NEW = ("orbfe_fuse_search", "orbfe_fuse_search_last_ms")
# the cases' point counts straddle the kernel's chunk, and the oracle speaks the entry's layout
assert (FC.CHUNK, O.KF_F64, O.PT_F64) == (LIB.ORBFE_FUSE_CHUNK, LIB.ORBFE_FUSE_KF_F64, LIB.ORBFE_FUSE_PT_F64)


def golden():
    return np.load(GOLDEN / "fuse_many.npz", allow_pickle=False)


# ---- the reference's golden ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", FC.N_NEIGH)
def test_oracle_and_replay_reproduce_the_reference(n):
    g = golden()
    w = FC.load_world(g)
    stats = {}
    got = FC.world_state(w, FC.drive(w, FC.oracle_fuse(stats), n))
    FC.assert_state(got, FC.golden_state(g, n), f"n = {n}")
    assert len(got["ret"]) == n + 1 and int(got["ret"].sum()) > 0
    if n == 6:  # what the generator searched seeds for
        log = got["log"]
        assert int((log[:, 0] == MW.EV_REPLACE).sum()) >= 20
        assert stats["list_replaced"] > 0 and stats["slot_replaced"] > 0
        assert stats["became_bad"] > 0 and stats["changed"] > 0 and stats["added"] > 0


def world_items(z):
    """The (keyframes, points) of both fusion calls of a fresh world, before any side effect."""
    w = MW.build(z)
    pts = [p for p in w.kfs[0].get_map_point_matches() if p is not None]
    yield w.kfs[1:], pts
    yield [w.kfs[0]], FC.pooled_points(w.kfs[1:])


@pytest.mark.parametrize("seed", [None, 11, 12, 13], ids=["golden", "seed11", "seed12", "seed13"])
def test_unmarked_items_decide_as_the_reference_and_few_are_marked(seed):
    """The soundness of the bound on float32 worlds: wherever the oracle leaves the status 0, its winner and
    distance are those of the reference's loop body on the objects.  At most 2 % of the items that reach a cell
    window may be marked (the generator measured 0.30 % on the golden world)."""
    z = golden() if seed is None else FC.Z(FC.clone_world(seed))
    reached = marked = found = 0
    for kfs, pts in world_items(z):
        a = O.pack(kfs, pts, FC.TH)
        assert a["eps"] == O.EPS_F32
        bi, bd, st = O.search(a)
        for k, kf in enumerate(kfs):
            for i, p in enumerate(pts):
                if O.reaches_candidates(a, k, i):
                    reached += 1
                    marked += int(st[k, i] != 0)
                if st[k, i]:
                    continue
                dist, idx = O.single_item(kf, p, FC.TH)
                assert (idx, dist if idx >= 0 else -1) == (int(bi[k, i]), int(bd[k, i])), (k, i)
                found += idx >= 0
    print(f"reached {reached} marked {marked} share {marked / reached:.4f} found {found}")
    assert reached > 1000 and found > 500
    assert marked <= 0.02 * reached


# ---- the crafted cases -------------------------------------------------------------------------------------------

CASES = FC.all_cases()
ORACLE = {c["name"]: FC.oracle(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_holds_its_claim(case):
    bi, bd, st = ORACLE[case["name"]]
    case["check"](bi, bd, st)
    assert bool(st.any()) == case["marginal"]
    assert bi.shape == bd.shape == st.shape == (len(case["frames"]), len(case["pt_f64"]))
    assert bool(((bi >= 0) == (bd >= 0)).all())


def test_the_set_is_not_vacuous():
    """Over the whole set a winner differs from what the search would take without the chi-square, without the
    octave filter, without the radius test, and with the last instead of the first of equal distances."""
    diff = {"chi_gate": 0, "octave_gate": 0, "radius_gate": 0, "early_tie": 0}
    for c in CASES:
        for k in diff:
            diff[k] += int((FC.oracle(c, **{k: False})[0] != ORACLE[c["name"]][0]).sum())
    assert all(v > 0 for v in diff.values()), diff
    names = {c["name"] for c in CASES}
    assert {f"points_{FC.CHUNK + d}" for d in (-1, 0, 1)} <= names
    for L in (1, 63, 64, 65, 129):  # that many entries pass every gate in one window
        c = next(c for c in CASES if c["name"] == f"window_{L}")
        assert len(c["frames"][0]["cell_idx"]) == L
        assert int((FC.oracle(c, chi_gate=False, octave_gate=False, radius_gate=False)[0] >= 0).sum()) == 2


# ---- the packer --------------------------------------------------------------------------------------------------

def test_packer_round_trips_and_refuses():
    from pyorbslam_amd import matcher
    w = FC.load_world(golden())
    for j in (0, 3):
        f, want = matcher._fuse_frame(w.kfs[j]), O.pack_kf(w.kfs[j])
        for k in ("f64", "i32", "xy", "octave", "u_right", "desc", "cell_off", "cell_idx", "scale", "inv_sigma2"):
            got = getattr(f, k)
            assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), (j, k)
        assert f.f32
    kf = w.kfs[1]
    first = matcher._fuse_frame(kf)
    assert matcher._fuse_frame(kf).xy is first.xy            # the static part is cached ...
    kf.Tcw = kf.Tcw.copy()
    kf.Tcw[0, 3] += 1.0
    assert matcher._fuse_frame(kf).f64[14] == float(kf.Tcw[0, 3]) != first.f64[14]   # ... the pose is read anew
    kf.mGrid = [list(col) for col in kf.mGrid]
    assert matcher._fuse_frame(kf).xy is not first.xy        # another grid object: packed again

    def refused(obj, name, value):
        keep = getattr(obj, name)
        setattr(obj, name, value)
        assert matcher._fuse_frame(kf) is None, name
        setattr(obj, name, keep)
        assert matcher._fuse_frame(kf) is not None, name
    refused(kf, "fx", np.float32(kf.fx))
    refused(kf, "mfGridElementWidthInv", np.float32(0.05))
    refused(kf, "mnMinX", 0)
    refused(kf, "mfLogScaleFactor", float("nan"))
    refused(kf, "mnScaleLevels", 0)
    refused(kf, "Tcw", kf.Tcw.astype(np.float16))
    bad = kf.Tcw.copy()
    bad[1, 1] = np.inf
    refused(kf, "Tcw", bad)
    refused(kf, "mvuRight", [np.float16(1.0)] * kf.N)
    refused(kf, "mvuRight", kf.mvuRight[:-1])
    refused(kf, "mvScaleFactors", [np.float32(1.2)] * 8)
    refused(kf, "mvInvLevelSigma2", [1.0] * 7)
    refused(kf, "mDescriptors", kf.mDescriptors.astype(np.int32))
    kp = kf.mvKeysUn[4]
    for name, value in (("pt", (np.float32(kp.pt[0]), kp.pt[1])), ("octave", 8), ("octave", -1), ("octave", 1.0)):
        keep = getattr(kp, name)
        setattr(kp, name, value)
        kf.mvKeysUn = list(kf.mvKeysUn)  # a new list: the cache does not answer
        assert matcher._fuse_frame(kf) is None, (name, value)
        setattr(kp, name, keep)
    kf.mvKeysUn = list(kf.mvKeysUn)
    assert matcher._fuse_frame(kf) is not None
    # a keyframe above the limit
    big = MW.KeyFrame(w, 9, MW.kf_arrays(np.random.Generator(np.random.PCG64(1)), 8193), np.eye(4))
    assert matcher._fuse_frame(big) is None
    # points
    p = w.mps[0]
    row = matcher._fuse_point(p)
    want = O.pack_point(p)
    assert row[0] == want[0] and np.array_equal(row[1], want[1]) and row[2] is True
    for name, value in (("_pos", p._pos.reshape(3)), ("_pos", p._pos.astype(np.float16)),
                        ("_normal", np.full((3, 1), np.nan, np.float32)), ("mfMaxDistance", np.float32(3.0)),
                        ("mDescriptor", p.mDescriptor[:31]), ("mDescriptor", p.mDescriptor.astype(np.int16))):
        keep = getattr(p, name)
        setattr(p, name, value)
        assert matcher._fuse_point(p) is None, name
        setattr(p, name, keep)
    assert matcher._fuse_point(p) is not None


def test_many_fall_back_without_a_launch(monkeypatch):
    """A th that is no plain number, keyframes the packer refuses, and an empty list: the loop's results, nothing is
    launched."""
    from pyorbslam_amd import matcher
    from test_matcher_kf import _cpu_batched
    monkeypatch.setattr(matcher.ORBMatcher, "_batched", staticmethod(_cpu_batched))
    monkeypatch.setattr(matcher, "fuse_search_arrays", lambda *a, **k: pytest.fail("launched"))
    g = golden()
    m = matcher.ORBMatcher()
    states = []
    for many in (False, True):
        w = FC.load_world(g)
        for kf in w.kfs[1:]:
            kf.fx = np.float32(kf.fx)
        pts = w.kfs[0].get_map_point_matches()
        ret = (m.fuse_pkf_mp_many(w.kfs[1:4], pts, FC.TH) if many
               else [m.fuse_pkf_mp(kf, pts, FC.TH) for kf in w.kfs[1:4]])
        states.append(FC.world_state(w, ret))
    FC.assert_state(states[1], states[0])
    assert int(states[0]["ret"].sum()) > 0
    states = []
    for many in (False, True):
        w = FC.load_world(g)
        pts = w.kfs[0].get_map_point_matches()
        th = np.float32(3.0)
        ret = m.fuse_pkf_mp_many(w.kfs[1:3], pts, th) if many else [m.fuse_pkf_mp(kf, pts, th) for kf in w.kfs[1:3]]
        states.append(FC.world_state(w, ret))
    FC.assert_state(states[1], states[0])
    w = FC.load_world(g)
    assert m.fuse_pkf_mp_many([], w.kfs[0].get_map_point_matches(), FC.TH) == []
    assert m.fuse_pkf_mp_many(w.kfs[1:3], [], FC.TH) == [0, 0] and m.fuse_pkf_mp_many(w.kfs[1:3], [None], FC.TH) == [0, 0]


def test_fuse_pkf_mp_still_equals_the_reference_golden(monkeypatch):
    """The loop body of fuse_pkf_mp was factored out for the single-item redo: the loop over the golden world still
    gives the reference's results."""
    from pyorbslam_amd import matcher
    from test_matcher_kf import _cpu_batched
    monkeypatch.setattr(matcher.ORBMatcher, "_batched", staticmethod(_cpu_batched))
    g = golden()
    m = matcher.ORBMatcher()
    w = FC.load_world(g)
    ret = FC.drive(w, lambda kfs, pts, th: [m.fuse_pkf_mp(kf, pts, th) for kf in kfs], 3)
    FC.assert_state(FC.world_state(w, ret), FC.golden_state(g, 3))


# ---- the ABI -------------------------------------------------------------------------------------------------------

def test_new_symbols_resolve_and_abi_is_still_9():
    from pyorbslam_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.orbfe_abi_version() == 9 == _lib.ORBFE_ABI_VERSION
    assert C.sizeof(_lib.FuseOut) == 3 * C.sizeof(C.c_void_p)


def test_table_and_header_agree():
    from pyorbslam_amd import _lib, matcher
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_fuse_out \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in _lib.FuseOut._fields_]
    for k in ("MARGINAL", "KF_F64", "PT_F64", "CHUNK"):
        assert int(re.search(rf"#define ORBFE_FUSE_{k} (\d+)", hdr).group(1)) == getattr(_lib, f"ORBFE_FUSE_{k}")
    assert (O.MARGINAL, O.KF_F64, O.PT_F64) == (_lib.ORBFE_FUSE_MARGINAL, _lib.ORBFE_FUSE_KF_F64, _lib.ORBFE_FUSE_PT_F64)
    assert FC.CHUNK == _lib.ORBFE_FUSE_CHUNK
    assert (O.EPS_F32, O.EPS_F64) == (matcher.FUSE_EPS_F32, matcher.FUSE_EPS_F64)
    assert int(re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1)) == 9


OUTS = ("best_idx", "best_dist", "status")


class HostCall:
    """orbfe_fuse_search over a small valid input (two keyframes, three points); each test breaks one thing."""

    def __init__(self):
        c = next(c for c in CASES if c["name"] == "ragged_2")
        self.a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in FC.arrays(c).items()}
        self.a["pt_f64"], self.a["pt_desc"] = self.a["pt_f64"][:3].copy(), self.a["pt_desc"][:3].copy()
        self.n_kf, self.n_pts, self.stride, self.th, self.eps = 2, 3, 3, FC.TH, O.EPS_F64
        self.o = dict(best_idx=np.full((2, 3), -7, np.int32), best_dist=np.full((2, 3), -7, np.int32),
                      status=np.full((2, 3), 7, np.uint8))
        self.null = set()

    def run(self):
        from pyorbslam_amd import _lib
        p = lambda k: None if k in self.null else _lib.ptr(self.a[k])  # noqa: E731
        out = _lib.FuseOut(**{k: None if k in self.null else v.ctypes.data for k, v in self.o.items()})
        rc = _lib.lib().orbfe_fuse_search(*[p(k) for k in O.ARRAYS[:14]], self.n_kf, p("pt_f64"), p("pt_desc"),
                                          self.n_pts, self.th, self.eps,
                                          None if "out" in self.null else C.byref(out), self.stride)
        return rc, _lib.lib().orbfe_last_error().decode()

    def untouched(self):
        return all(bool((x == (7 if k == "status" else -7)).all()) for k, x in self.o.items())


def refused(h, *words):
    from pyorbslam_amd import _lib
    rc, msg = h.run()
    assert rc == _lib.ORBFE_EINVAL and all(w in msg for w in words), (rc, msg)
    assert "ORBFE_" not in msg and h.untouched()


@pytest.mark.parametrize("name", O.ARRAYS + ("out",) + OUTS)
def test_required_pointers(name):
    h = HostCall()
    h.null.add(name)
    refused(h, "null argument")


def test_offsets_limits_and_stride():
    from pyorbslam_amd import _lib
    for k in ("off", "cell_at", "idx_at", "lvl_off"):
        h = HostCall()
        h.a[k][0] = 1
        refused(h, "must be 0")
        h = HostCall()
        h.a[k][1], h.a[k][2] = h.a[k][2] + 1, h.a[k][2]
        refused(h, "keyframe 1", "must not decrease")
    h = HostCall()
    h.a["off"] = np.array([0, _lib.ORBFE_BOW_MAX_FRAME + 1, _lib.ORBFE_BOW_MAX_FRAME + 5], np.int64)
    refused(h, "keyframe 0", f"limit of {_lib.ORBFE_BOW_MAX_FRAME} per keyframe")
    h = HostCall()
    h.stride = 2
    refused(h, "out_stride", "below the point count")
    for kw in (dict(n_kf=-1), dict(n_pts=-1), dict(stride=-1), dict(n_kf=65536)):
        h = HostCall()
        for k, v in kw.items():
            setattr(h, k, v)
        assert h.run()[0] == _lib.ORBFE_EINVAL and h.untouched()


def test_grid_checks():
    h = HostCall()
    h.a["cell_at"][1:] = [1200, 2401]
    refused(h, "keyframe 0", "columns * rows + 1")
    h = HostCall()
    h.a["kf_i32"][1, 0] = 0
    refused(h, "keyframe 1", "columns and rows")
    h = HostCall()
    h.a["cell_off"][5] = 1          # decreases at the next cell
    refused(h, "keyframe 0", "cell offsets must not decrease")
    h = HostCall()
    h.a["cell_off"][0] = 1
    refused(h, "keyframe 0", "first cell offset")
    h = HostCall()
    h.a["cell_off"][1200] = 2       # keyframe 0's last offset: it has one grid entry
    refused(h, "keyframe 0", "last cell offset")
    for v in (4, -1):               # keyframe 1 has four features
        h = HostCall()
        h.a["cell_idx"][2] = v
        refused(h, "keyframe 1", "grid entry", "outside")


def test_levels_octaves_and_finiteness():
    for v in (0, -3):
        h = HostCall()
        h.a["kf_i32"][1, 2] = v
        refused(h, "keyframe 1", "level count")
    h = HostCall()
    h.a["kf_i32"][0, 2] = 3
    refused(h, "keyframe 0", "one entry per level")
    for v in (4, -1):
        h = HostCall()
        h.a["octave"][2] = v
        refused(h, "keyframe 1", "octave")
    for v in (np.nan, np.inf, -np.inf):
        for col in (0, 5, 16, 19, 20, 24, 26):
            h = HostCall()
            h.a["kf_f64"][1, col] = v
            refused(h, "keyframe 1", "scalar", "finite")
        h = HostCall()
        h.a["xy"][3, 1] = v
        refused(h, "keyframe 1", "coordinate", "finite")
        h = HostCall()
        h.a["u_right"][0] = v
        refused(h, "keyframe 0", "coordinate", "finite")
        h = HostCall()
        h.a["scale"][5] = v
        refused(h, "keyframe 1", "level table", "finite")
        h = HostCall()
        h.a["inv_sigma2"][1] = v
        refused(h, "keyframe 0", "level table", "finite")
        h = HostCall()
        h.a["pt_f64"][2, 8] = v
        refused(h, "point scalar", "finite")
        h = HostCall()
        h.th = v
        refused(h, "th and eps")
        h = HostCall()
        h.eps = v
        refused(h, "th and eps")
    h = HostCall()
    h.eps = -1e-9
    refused(h, "th and eps")


def test_nothing_to_do_needs_no_device():
    h = HostCall()
    h.n_kf = 0
    assert h.run()[0] == 0 and h.untouched()
    h = HostCall()
    h.n_pts = 0
    assert h.run()[0] == 0 and h.untouched()
    h = HostCall()
    h.n_kf, h.null = 0, set(O.ARRAYS) | {"out"}
    assert h.run()[0] == 0
