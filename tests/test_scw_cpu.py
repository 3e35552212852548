"""Loop closing's Sim3 projection searches without a GPU: the claims of the placed cases, the array oracle and both
replays against the golden made by the reference itself (tests/golden/gen_golden_scw.py), the soundness of the error
bound, the fallbacks that need no launch, the new symbols, and every argument check of orbfe_scw_search, all of which
come before any device call."""
import ctypes as C
import re

import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as O
import matcher_world as MW
import scw_cases as SC
import scw_oracle as SO
from conftest import GOLDEN, ROOT
from pyorbslam_amd import _lib as LIB

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")
NEW = ("orbfe_scw_search", "orbfe_scw_search_last_ms")
assert (SC.CHUNK, SO.KF_F64, SO.PT_F64) == (LIB.ORBFE_FUSE_CHUNK, LIB.ORBFE_FUSE_KF_F64, LIB.ORBFE_FUSE_PT_F64)


def golden():
    return np.load(GOLDEN / "scw_many.npz", allow_pickle=False)


# ---- the placed cases ----------------------------------------------------------------------------------------------

CASES = SC.all_cases()
ORACLE = {c["name"]: SC.oracle(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_holds_its_claim(case):
    bi, bd, st = ORACLE[case["name"]]
    case["check"](bi, bd, st)
    assert bool(st.any()) == case["marginal"]
    assert bi.shape == bd.shape == st.shape == (len(case["frames"]), len(case["pt_f64"]))
    assert bool(((bi >= 0) == (bd >= 0)).all())


def test_the_set_is_not_vacuous():
    """Over the whole set a winner differs from what the search would take without the blocked bytes, without the
    octave filter, without the radius test, and with the last instead of the first of equal distances; and the
    sizes the kernel's loops turn at are there."""
    diff = {"blocked_mask": 0, "octave_gate": 0, "radius_gate": 0, "early_tie": 0}
    for c in CASES:
        for k in diff:
            diff[k] += int((SC.oracle(c, **{k: False})[0] != ORACLE[c["name"]][0]).sum())
    assert all(v > 0 for v in diff.values()), diff
    names = {c["name"] for c in CASES}
    assert {f"points_{P}" for P in (SC.CHUNK - 1, SC.CHUNK, SC.CHUNK + 1, 2 * SC.CHUNK + 1)} <= names
    for L in (SC.GROUP - 1, SC.GROUP, SC.GROUP + 1):  # that many entries pass every gate in one window
        c = next(c for c in CASES if c["name"] == f"window_{L}")
        assert len(c["frames"][0]["cell_idx"]) == L
        assert int((SC.oracle(c, octave_gate=False, radius_gate=False)[0] >= 0).sum()) == 2
    assert {"keyframe_without_features", "zero_points", "no_keyframes", "ragged_9", "octave_window"} <= names
    assert sum(c["blocked"] is not None for c in CASES) >= 5 and sum(c["eps"] == SO.EPS_F32 for c in CASES) >= 2


# ---- the reference's golden ------------------------------------------------------------------------------------

def oracle_many(stats=None):
    return lambda kfs, S, pts, th, after: SO.replay_fuse(kfs, S, pts, th, after, stats=stats)


@pytest.mark.parametrize("n,prefix", [(1, "n"), (3, "n"), (6, "n"), (6, "p")])
def test_oracle_and_replay_reproduce_the_reference_fusion(n, prefix):
    g = golden()
    w = MW.build(g)
    stats = {}
    got = SC.fuse_state(w, SC.drive_fuse(w, g, oracle_many(stats), n, after=prefix == "n"))
    SC.assert_state(got, SC.golden_state(g, n, prefix), f"{prefix}{n}")
    assert len(got["ret"]) == n and int(got["ret"].sum()) > 0
    assert stats["marginal"] <= 0.02 * stats["reached"]
    if (n, prefix) == (6, "n"):  # what the generator searched seeds for
        assert int((got["log"][:, 0] == MW.EV_REPLACE).sum()) >= 20
        assert stats["already_later"] > 0 and stats["changed"] > 0 and stats["added"] > 0 and stats["replaced"] >= 20
    if prefix == "p":
        assert int((got["log"][:, 0] == MW.EV_REPLACE).sum()) == 0 and int((got["rep"] >= 0).sum()) > 0


def test_oracle_and_replay_reproduce_the_reference_ckf():
    g = golden()
    stats = {}
    n, vm = SC.drive_ckf(MW.build(g), g, lambda kf, S, pts, m, th: SO.replay_ckf(kf, S, pts, m, th, stats=stats))
    assert n == int(g["ckf_n"]) > 20 and np.array_equal(vm, g["ckf_matched"])
    assert stats["taken"] > 0 and stats["marginal"] <= 0.02 * stats["reached"]
    pre = g["ckf_pre"]
    assert 0.25 < float((pre >= 0).mean()) < 0.4 and np.array_equal(vm[pre >= 0], pre[pre >= 0])


@pytest.mark.parametrize("seed", [None, 21, 22], ids=["golden", "seed21", "seed22"])
def test_unmarked_items_decide_as_the_reference_and_few_are_marked(seed):
    """The soundness of the bound on float32 worlds with float64 and float32 Scw: wherever the oracle leaves the
    status 0, its winner and distance are those of the reference's loop body on the objects, in both searches.  At
    most 2 % of the items that reach a cell window may be marked."""
    z = golden() if seed is None else FC.Z(FC.clone_world(seed))
    w = MW.build(z)
    pts = SC.loop_points(w)
    reached = marked = found = 0
    for dtype in (np.float64, np.float32):
        kfs = w.kfs[1:]
        Scws = [MW.sim3(kf.Tcw, s).astype(dtype) for kf, s in zip(kfs, SC.SCALES * 2)]
        for th, pose, vm in ((SC.TH_FUSE, SO.fuse_pose, None), (SC.TH_CKF, SO.ckf_pose, [None] * kfs[0].N)):
            a = SO.pack(kfs, Scws, pts, th, None, pose)
            assert a["eps"] == SO.EPS_F32
            bi, bd, st = SO.search(a)
            for k, kf in enumerate(kfs):
                P = pose(Scws[k])
                for i, p in enumerate(pts):
                    if SO.reaches_candidates(a, k, i):
                        reached += 1
                        marked += int(st[k, i] != 0)
                    if st[k, i]:
                        continue
                    dist, idx = SO.single_item(kf, p, P, th, vm)
                    assert (idx, dist if idx >= 0 else -1) == (int(bi[k, i]), int(bd[k, i])), (k, i)
                    found += idx >= 0
    print(f"reached {reached} marked {marked} share {marked / reached:.4f} found {found}")
    assert reached > 1000 and found > 500
    assert marked <= 0.02 * reached


# ---- fallbacks that need no launch -----------------------------------------------------------------------------------

def cpu_matcher(monkeypatch):
    from pyorbslam_amd import matcher
    from test_matcher_kf import _cpu_batched
    monkeypatch.setattr(matcher.ORBMatcher, "_batched", staticmethod(_cpu_batched))
    monkeypatch.setattr(matcher, "scw_search_arrays", lambda *a, **k: pytest.fail("launched"))
    return matcher.ORBMatcher()


def oracle_device(monkeypatch, launches):
    """The product with the array oracle in the device's place: scw_search_arrays answers from scw_oracle.search."""
    from pyorbslam_amd import matcher
    from test_matcher_kf import _cpu_batched

    def arrays(*a):
        d = dict(zip(SO.ARRAYS + ("th", "eps"), a))
        for k in ("kf_f64", "pt_f64"):
            d[k] = np.asarray(d[k], np.float64).reshape(-1, SO.KF_F64 if k == "kf_f64" else SO.PT_F64)
        d["xy"] = np.asarray(d["xy"]).reshape(-1, 2)
        d["desc"], d["pt_desc"] = np.asarray(d["desc"]).reshape(-1, 32), np.asarray(d["pt_desc"]).reshape(-1, 32)
        launches.append((len(d["kf_f64"]), len(d["pt_f64"])))
        bi, bd, st = SO.search(d)
        return dict(best_idx=bi, best_dist=bd, status=st)
    monkeypatch.setattr(matcher.ORBMatcher, "_batched", staticmethod(_cpu_batched))
    monkeypatch.setattr(matcher, "scw_search_arrays", arrays)
    monkeypatch.setattr(matcher._lib, "device_present", lambda: True)
    return matcher.ORBMatcher()


@pytest.mark.parametrize("n,prefix", [(3, "n"), (6, "n"), (6, "p")])
def test_the_products_replay_over_the_oracles_answers_equals_the_golden(monkeypatch, n, prefix):
    """fuse_kf_scw_mp_many's packing and ordered replay, with the oracle answering for the kernel: one launch, the
    reference's state."""
    launches = []
    m = oracle_device(monkeypatch, launches)
    g = golden()
    w = MW.build(g)
    got = SC.fuse_state(w, SC.drive_fuse(w, g, m.fuse_kf_scw_mp_many, n, after=prefix == "n"))
    SC.assert_state(got, SC.golden_state(g, n, prefix))
    assert launches == [(n, sum(1 for p in SC.loop_points(MW.build(g)) if not p.is_bad()))]


def test_the_products_ckf_replay_over_the_oracles_answers_equals_the_golden(monkeypatch):
    launches = []
    m = oracle_device(monkeypatch, launches)
    monkeypatch.setattr(m, "_ckf_host", lambda *a: pytest.fail("host body"))
    singles, one = [], m._scw_one
    monkeypatch.setattr(m, "_scw_one", lambda *a: singles.append(1) or one(*a))
    g = golden()
    n, vm = SC.drive_ckf(MW.build(g), g, m.search_by_projection_ckf_scw_mp)
    assert n == int(g["ckf_n"]) and np.array_equal(vm, g["ckf_matched"])
    stats = {}
    SC.drive_ckf(MW.build(g), g, lambda kf, S, pts, v, th: SO.replay_ckf(kf, S, pts, v, th, stats=stats))
    assert len(launches) == 1 and launches[0][0] == 1 and len(singles) == stats["taken"] > 0


BAD_SCW = [lambda S: S.astype(np.float16), lambda S: S[:3], lambda S: S.tolist(),
           lambda S: np.where(np.arange(16).reshape(4, 4) == 7, np.inf, S),
           lambda S: np.where(np.arange(16).reshape(4, 4) < 3, 0.0, S)]


def test_many_fall_back_without_a_launch(monkeypatch):
    """Keyframes the packer refuses, a th that is no plain number, unacceptable Scw and empty lists: the loop's
    results, nothing is launched."""
    m = cpu_matcher(monkeypatch)
    g = golden()

    def both(prepare, th=SC.TH_FUSE, n=3):
        states = []
        for many in (False, True):
            w = MW.build(g)
            prepare(w)
            pts = SC.loop_points(w)
            fuse = m.fuse_kf_scw_mp_many if many else SC.loop_fuse(m.fuse_kf_scw_mp)
            states.append(SC.fuse_state(w, fuse(w.kfs[1:1 + n], SC.scws(g, n), pts, th, SC.replacer(pts))))
        SC.assert_state(states[1], states[0])
        return states[0]

    def refuse_all(w):
        for kf in w.kfs[1:]:
            kf.fx = np.float32(kf.fx)
    s = both(refuse_all)
    assert int(s["ret"].sum()) > 0 and int((s["log"][:, 0] == MW.EV_REPLACE).sum()) > 0
    SC.assert_state(both(lambda w: None, th=np.float32(4.0)), SC.golden_state(g, 3))
    w = MW.build(g)
    pts = SC.loop_points(w)
    assert m.fuse_kf_scw_mp_many([], [], pts, SC.TH_FUSE) == []
    assert m.fuse_kf_scw_mp_many(w.kfs[1:3], SC.scws(g, 2), [], SC.TH_FUSE) == [(0, []), (0, [])]
    with pytest.raises(ValueError):
        m.fuse_kf_scw_mp_many(w.kfs[1:3], SC.scws(g, 1), pts, SC.TH_FUSE)
    for bad in BAD_SCW[:1] + BAD_SCW[3:]:   # those the reference itself can compute with
        states = []
        for many in (False, True):
            w = MW.build(g)
            pts = SC.loop_points(w)
            S = [bad(np.asarray(x)) for x in SC.scws(g, 2)]
            fuse = m.fuse_kf_scw_mp_many if many else SC.loop_fuse(m.fuse_kf_scw_mp)
            with np.errstate(all="ignore"):
                states.append(SC.fuse_state(w, fuse(w.kfs[1:3], S, pts, SC.TH_FUSE, SC.replacer(pts))))
        SC.assert_state(states[1], states[0])


def test_scw_frame_refusals():
    from pyorbslam_amd import matcher
    g = golden()
    w = MW.build(g)
    S = np.asarray(g["Scw1"])
    M = matcher.ORBMatcher
    f, pose = M._scw_frame(w.kfs[1], S, M._sim3_to_pose)
    want = SO.with_pose(O.pack_kf(w.kfs[1]), SO.fuse_pose(S))
    assert np.array_equal(f.f64, want["f64"]) and not f.f32 and all(np.array_equal(a, b) for a, b in zip(pose, SO.fuse_pose(S)))
    assert M._scw_frame(w.kfs[1], S.astype(np.float32), M._ckf_pose)[0].f32
    for bad in BAD_SCW:
        assert M._scw_frame(w.kfs[1], bad(S), M._sim3_to_pose) is None
    tiny = S.copy()
    tiny[:3] *= 1e-320   # a first row that is not zero but whose division overflows
    assert M._scw_frame(w.kfs[1], tiny, M._sim3_to_pose) is None
    w.kfs[1].fx = np.float32(w.kfs[1].fx)
    assert M._scw_frame(w.kfs[1], S, M._sim3_to_pose) is None


def test_ckf_host_body_equals_the_goldens(monkeypatch):
    """The former body of search_by_projection_ckf_scw_mp, now the fallback: the keyframe-level goldens and this
    file's run (b), by the private method and by the public one where nothing can be launched."""
    m = cpu_matcher(monkeypatch)
    g = golden()
    for search in (m._ckf_host, m.search_by_projection_ckf_scw_mp):
        n, vm = SC.drive_ckf(MW.build(g), g, search)
        assert n == int(g["ckf_n"]) and np.array_equal(vm, g["ckf_matched"])
    for case in (0, 5):
        z = np.load(GOLDEN / f"matcher_kf_{case}.npz", allow_pickle=False)
        w = MW.build(z)
        s = [1.0, 1.3, 0.8, 2.0, 1.1, 1.0, 1.0][case]
        th = [3.0, 5.0, 8.0, 4.0, 3.0, 10.0, 10.0][case]
        pts = [w.mps[i] for i in z["sel_ckf_pts"]]
        vm = [None if i < 0 else w.mps[i] for i in z["sel_ckf_matched"]]
        n, vm = m._ckf_host(w.kfs[1], MW.sim3(z["kf1_T"], s), pts, vm, th)
        assert n == int(z["ckf_n"]) and np.array_equal(MW.encode_mps(w, vm), z["ckf_matched"])


def test_ckf_refusals_take_the_host_body(monkeypatch):
    """With a device present the public method still takes the host body for a th that is no plain number, an
    unacceptable Scw, a refused keyframe and a vpMatched of another length."""
    from pyorbslam_amd import matcher
    m = cpu_matcher(monkeypatch)
    monkeypatch.setattr(matcher._lib, "device_present", lambda: True)
    g = golden()
    calls = []
    host = m._ckf_host
    monkeypatch.setattr(m, "_ckf_host", lambda *a: calls.append(1) or host(*a))
    w = MW.build(g)
    kf, S, pts = w.kfs[1], np.asarray(g["ckf_Scw"]), list(w.mps)
    vm = lambda: [None if i < 0 else w.mps[int(i)] for i in g["ckf_pre"]]  # noqa: E731
    want = int(g["ckf_n"])
    assert m.search_by_projection_ckf_scw_mp(kf, S, pts, vm(), np.float32(SC.TH_CKF))[0] == want
    assert m.search_by_projection_ckf_scw_mp(kf, S.astype(np.float16), pts, vm(), SC.TH_CKF)[0] > 0
    assert m.search_by_projection_ckf_scw_mp(kf, S, pts, vm() + [None], SC.TH_CKF)[0] == want
    kf.fx = np.float32(kf.fx)
    assert m.search_by_projection_ckf_scw_mp(kf, S, pts, vm(), SC.TH_CKF)[0] > 0
    assert len(calls) == 4


# ---- the ABI -------------------------------------------------------------------------------------------------------

def test_new_symbols_resolve_and_abi_is_still_9():
    L = LIB.lib()
    for name in NEW:
        assert name in LIB.SIGNATURES and getattr(L, name) is not None
    assert L.orbfe_abi_version() == 9 == LIB.ORBFE_ABI_VERSION
    assert C.sizeof(LIB.ScwOut) == 3 * C.sizeof(C.c_void_p)


def test_table_and_header_agree():
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(LIB.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_scw_out \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in LIB.ScwOut._fields_]
    assert int(re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1)) == 9
    # the Makefile builds the file that defines the entry
    src = ROOT / "pyorbslam_amd" / "csrc" / "orbfe_fuse.hip"
    assert re.search(r"^int orbfe_scw_search\s*\(", src.read_text(), flags=re.M)
    assert "pyorbslam_amd/csrc/orbfe_fuse.hip" in (ROOT / "Makefile").read_text()


OUTS = ("best_idx", "best_dist", "status")
OPTIONAL = ("blocked",)


class HostCall:
    """orbfe_scw_search over a small valid input (two keyframes, three points); each test breaks one thing."""

    def __init__(self):
        c = next(c for c in CASES if c["name"] == "ragged_2")
        self.a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in SC.arrays(c).items()}
        self.a["pt_f64"], self.a["pt_desc"] = self.a["pt_f64"][:3].copy(), self.a["pt_desc"][:3].copy()
        self.a["blocked"] = np.zeros(int(self.a["off"][-1]), np.uint8)
        self.n_kf, self.n_pts, self.stride, self.th, self.eps = 2, 3, 3, SC.TH, SO.EPS_F64
        self.o = dict(best_idx=np.full((2, 3), -7, np.int32), best_dist=np.full((2, 3), -7, np.int32),
                      status=np.full((2, 3), 7, np.uint8))
        self.null = set()

    def run(self):
        p = lambda k: None if k in self.null else LIB.ptr(self.a[k])  # noqa: E731
        out = LIB.ScwOut(**{k: None if k in self.null else v.ctypes.data for k, v in self.o.items()})
        rc = LIB.lib().orbfe_scw_search(*[p(k) for k in SO.ARRAYS[:13]], self.n_kf, p("pt_f64"), p("pt_desc"),
                                        self.n_pts, self.th, self.eps,
                                        None if "out" in self.null else C.byref(out), self.stride)
        return rc, LIB.lib().orbfe_last_error().decode()

    def untouched(self):
        return all(bool((x == (7 if k == "status" else -7)).all()) for k, x in self.o.items())


def refused(h, *words):
    rc, msg = h.run()
    assert rc == LIB.ORBFE_EINVAL and all(w in msg for w in words), (rc, msg)
    assert "ORBFE_" not in msg and h.untouched()


@pytest.mark.parametrize("name", tuple(k for k in SO.ARRAYS if k not in OPTIONAL) + ("out",) + OUTS)
def test_required_pointers(name):
    h = HostCall()
    h.null.add(name)
    refused(h, "null argument")


def test_offsets_limits_and_stride():
    for k in ("off", "cell_at", "idx_at", "lvl_off"):
        h = HostCall()
        h.a[k][0] = 1
        refused(h, "must be 0")
        h = HostCall()
        h.a[k][1], h.a[k][2] = h.a[k][2] + 1, h.a[k][2]
        refused(h, "keyframe 1", "must not decrease")
    h = HostCall()
    h.a["off"] = np.array([0, LIB.ORBFE_BOW_MAX_FRAME + 1, LIB.ORBFE_BOW_MAX_FRAME + 5], np.int64)
    refused(h, "keyframe 0", f"limit of {LIB.ORBFE_BOW_MAX_FRAME} per keyframe")
    h = HostCall()
    h.stride = 2
    refused(h, "out_stride", "below the point count")
    for kw in (dict(n_kf=-1), dict(n_pts=-1), dict(stride=-1), dict(n_kf=65536)):
        h = HostCall()
        for k, v in kw.items():
            setattr(h, k, v)
        assert h.run()[0] == LIB.ORBFE_EINVAL and h.untouched()


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
        for col in (0, 3, 5, 16, 19, 20, 24, 26):
            h = HostCall()
            h.a["kf_f64"][1, col] = v
            refused(h, "keyframe 1", "scalar", "finite")
        h = HostCall()
        h.a["xy"][3, 1] = v
        refused(h, "keyframe 1", "coordinate", "finite")
        h = HostCall()
        h.a["scale"][5] = v
        refused(h, "keyframe 1", "level table", "finite")
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
    h.n_kf, h.null = 0, set(SO.ARRAYS) | {"out"}
    assert h.run()[0] == 0
