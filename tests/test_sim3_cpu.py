"""k_sim3_search without a device: the placed cases against the array oracle, the oracle against the reference's
golden, the product's packing with the oracle in the kernel's place, the fallbacks, the ABI and every validation path
of orbfe_sim3_search (all of which return before the first device call)."""
import ctypes as C
import re

import numpy as np
import pytest

import fuse_cases as FC
import matcher_world as MW
import sim3_cases as SC
import sim3_oracle as S3
from conftest import GOLDEN, ROOT
from pyorbslam_amd import _lib as LIB

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")
NEW = ("orbfe_sim3_search", "orbfe_sim3_search_last_ms")


def golden():
    return np.load(GOLDEN / "sim3_many.npz", allow_pickle=False)


CASES = SC.all_cases()
ORACLE = {c["name"]: SC.oracle(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_holds_its_claim(case):
    bi, bd, st = ORACLE[case["name"]]
    case["check"](bi, bd, st)
    assert np.flatnonzero(st).tolist() == case["marked"]
    assert bi.dtype == bd.dtype == np.int32 and st.dtype == np.uint8 and len(bi) == sum(map(len, case["items"]))


def _differs(name, **switch):
    c = SC.by_name(name)
    a, b = ORACLE[name], SC.oracle(c, **switch)
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_the_set_is_not_vacuous():
    """Each property of the mode, turned off in the oracle, changes the answer of the case built for it."""
    assert _differs("two_stage_pose", one_stage=1) and _differs("two_stage_pose", one_stage=2)
    assert _differs("intrinsics_from_the_search", target_intrinsics=True)
    assert _differs("scale_changes_the_level", world_distance=True)
    bi = SC.oracle(SC.by_name("scale_changes_the_level"), world_distance=True)[0]
    assert bi.tolist() == [0]   # the closer feature of octave 1, which only level 1 takes
    assert _differs("normal_pointing_away_still_matches", viewing_gate=True)
    assert SC.oracle(SC.by_name("normal_pointing_away_still_matches"), viewing_gate=True)[0].tolist() == [-1]
    assert _differs("shared_points", identity_items=True) and _differs("ragged_0_1_255_256_257", identity_items=True)
    for name in ("fuse_tie_in_two_cells", "fuse_tie_in_one_unsorted_cell", "fuse_window_65"):
        assert _differs(name, early_tie=False)
    marked = [c["name"] for c in CASES if c["marked"]]
    assert marked == ["dist_at_min", "dist_at_max", "marginal"]
    sizes = [len(it) for it in SC.by_name("ragged_0_1_255_256_257")["items"]]
    assert sizes == [1, 0, 255, 256, 0, 257, 0]
    assert SC.by_name("eps_of_float32")["eps"] == S3.EPS_F32


# ---- the oracle against the reference ----------------------------------------------------------------------------------

def oracle_many(stats=None, agree=False):
    return lambda kf1, kfs2, vs, ss, Rs, ts, th: S3.replay(kf1, list(zip(kfs2, vs, ss, Rs, ts)), th, stats=stats,
                                                            agree=agree)


def golden_results(g, n):
    return [int(g[f"sim3_n{j}"]) for j in range(1, n + 1)], [g[f"sim3_matches{j}"] for j in range(1, n + 1)]


def same(got, want):
    return got[0] == want[0] and len(got[1]) == len(want[1]) and all(np.array_equal(a, b) for a, b in zip(*(got[1], want[1])))


def test_oracle_and_redo_reproduce_the_reference():
    g = golden()
    stats = {}
    got = SC.drive(MW.build(g), g, oracle_many(stats), 6)
    assert same(got, golden_results(g, 6))
    assert max(got[0]) >= 20 and stats["refused"] > 0 and stats["marginal"] <= 0.02 * stats["reached"]


@pytest.mark.parametrize("seed", [None, 31, 32], ids=["golden", "seed31", "seed32"])
def test_unmarked_items_decide_as_the_reference_and_few_are_marked(seed):
    """The soundness of the two-stage bound on float32 worlds with float64 and float32 Sim3 parts: wherever the
    oracle leaves the status 0, its winner and distance are those of the reference's loop body on the objects, in both
    directions.  At most 2 % of the items that reach a cell window may be marked."""
    z = golden() if seed is None else FC.Z(FC.clone_world(seed))
    reached = marked = items = 0
    for dtype in (np.float64, np.float32):
        w = MW.build(z)
        g = SC.make_sim3s(w, 77 if seed is None else seed, dtype)
        stats = {}
        SC.drive(w, g, oracle_many(stats, agree=True), 6)
        reached, marked, items = reached + stats["reached"], marked + stats["marginal"], items + stats["items"]
    print(f"items {items} reached {reached} marked {marked} share {marked / reached:.4f}")
    assert reached > 1000
    assert marked <= 0.02 * reached


# ---- the product's packing, with the oracle in the kernel's place ---------------------------------------------------

def oracle_device(monkeypatch, launches, present=True):
    from pyorbslam_amd import matcher
    from test_matcher_kf import _cpu_batched

    def arrays(*a):
        d = dict(zip(S3.ARRAYS + ("th", "eps"), a))
        d["kf_f64"] = np.asarray(d["kf_f64"], np.float64).reshape(-1, S3.KF_F64)
        d["kf_i32"] = np.asarray(d["kf_i32"]).reshape(-1, 3)
        d["pt_f64"] = np.asarray(d["pt_f64"], np.float64).reshape(-1, S3.PT_F64)
        d["srch_f64"] = np.asarray(d["srch_f64"], np.float64).reshape(-1, S3.SIM3_F64)
        d["xy"] = np.asarray(d["xy"]).reshape(-1, 2)
        d["desc"], d["pt_desc"] = np.asarray(d["desc"]).reshape(-1, 32), np.asarray(d["pt_desc"]).reshape(-1, 32)
        launches.append((len(d["kf_f64"]), len(d["srch_f64"]), len(d["pt_f64"]), d["eps"]))
        bi, bd, st = S3.search(d)
        return dict(best_idx=bi, best_dist=bd, status=st)
    monkeypatch.setattr(matcher.ORBMatcher, "_batched", staticmethod(_cpu_batched))
    monkeypatch.setattr(matcher, "sim3_search_arrays", arrays)
    monkeypatch.setattr(matcher._lib, "device_present", lambda: present)
    return matcher.ORBMatcher()


@pytest.mark.parametrize("n", SC.N_PAIRS)
def test_the_products_packing_over_the_oracles_answers_equals_the_golden(monkeypatch, n):
    """search_by_sim3_many's packing and application with the oracle answering for the kernel: one launch of 2 n
    searches over n + 1 keyframes, pKF1's live points sent once, the reference's results."""
    launches = []
    m = oracle_device(monkeypatch, launches)
    monkeypatch.setattr(m, "_sim3_host", lambda *a: pytest.fail("host body"))
    g = golden()
    w = MW.build(g)
    prs = SC.pairs_of(w, g, n)
    lists = [p[1] for p in prs]
    res = m.search_by_sim3_many(w.kfs[0], *[[p[c] for p in prs] for c in range(5)], SC.TH_SIM3)
    assert same(SC.encode(w, res), golden_results(g, n))
    assert all(type(r) is tuple and type(r[0]) is int and r[1] is v for r, v in zip(res, lists))
    a, _ = S3.pack(MW.build(g).kfs[0], SC.pairs_of(MW.build(g), g, n), SC.TH_SIM3)
    assert launches == [(n + 1, 2 * n, len(a["pt_f64"]), S3.EPS_F32)]
    launches.clear()
    one = SC.drive(MW.build(g), g, SC.loop_single(m.search_by_sim3), n)
    assert same(one, golden_results(g, n)) and len(launches) == n


def test_marked_and_inexpressible_items_go_alone(monkeypatch):
    """Every tenth item forced marginal, and a point with a float32 mfMaxDistance: the golden still, with exactly
    those items redone alone."""
    from pyorbslam_amd import matcher
    launches = []
    m = oracle_device(monkeypatch, launches)
    inner = matcher.sim3_search_arrays
    forced = []

    def arrays(*a):
        r = inner(*a)
        forced.append(int(np.count_nonzero(r["status"][::10] == 0)) + int(np.count_nonzero(r["status"])))
        r["status"][::10] = S3.MARGINAL
        return r
    monkeypatch.setattr(matcher, "sim3_search_arrays", arrays)
    singles, one = [], m._sim3_one
    monkeypatch.setattr(m, "_sim3_one", lambda *a: singles.append(a[0]) or one(*a))
    g = golden()
    w = MW.build(g)
    odd = next(p for p in w.kfs[0].mvpMapPoints if p is not None and not p.is_bad())
    odd.mfMaxDistance = np.float32(odd.mfMaxDistance)
    prs = SC.pairs_of(w, g, 3)
    res = m.search_by_sim3_many(w.kfs[0], *[[p[c] for p in prs] for c in range(5)], SC.TH_SIM3)
    w2 = MW.build(g)
    next(p for p in w2.kfs[0].mvpMapPoints if p is not None and not p.is_bad()).mfMaxDistance = odd.mfMaxDistance
    want = SC.drive(w2, g, SC.loop_single(m._sim3_host), 3)
    assert same(SC.encode(w, res), want)
    alone = sum(1 for p in prs if not p[1][w.kfs[0].mvpMapPoints.index(odd)])
    assert len(launches) == 1 and len(singles) == forced[0] + alone and sum(p is odd for p in singles) == alone > 0


# ---- fallbacks -------------------------------------------------------------------------------------------------------

def cpu_matcher(monkeypatch, present=False):
    from pyorbslam_amd import matcher
    from test_matcher_kf import _cpu_batched
    monkeypatch.setattr(matcher.ORBMatcher, "_batched", staticmethod(_cpu_batched))
    monkeypatch.setattr(matcher, "sim3_search_arrays", lambda *a, **k: pytest.fail("launched"))
    monkeypatch.setattr(matcher._lib, "device_present", lambda: present)
    return matcher.ORBMatcher()


def test_without_a_device_the_host_body_runs_and_equals_the_golden(monkeypatch):
    m = cpu_matcher(monkeypatch)
    g = golden()
    for single in (m._sim3_host, m.search_by_sim3):
        assert same(SC.drive(MW.build(g), g, SC.loop_single(single), 6), golden_results(g, 6))
    w = MW.build(g)
    prs = SC.pairs_of(w, g, 6)
    lists = [p[1] for p in prs]
    res = m.search_by_sim3_many(w.kfs[0], *[[p[c] for p in prs] for c in range(5)], SC.TH_SIM3)
    assert same(SC.encode(w, res), golden_results(g, 6)) and all(r[1] is v for r, v in zip(res, lists))
    assert m.search_by_sim3_many(w.kfs[0], [], [], [], [], [], SC.TH_SIM3) == []
    with pytest.raises(ValueError):
        m.search_by_sim3_many(w.kfs[0], w.kfs[1:3], [[], []], [1.0], [np.eye(3)] * 2, [np.zeros((3, 1))] * 2, 7.5)


REFUSALS = {
    "kf1 refused": lambda w, a: setattr(w.kfs[0], "fx", np.float32(w.kfs[0].fx)),
    "kf2 refused": lambda w, a: setattr(w.kfs[1], "fy", np.float32(w.kfs[1].fy)),
    "R12 float16": lambda w, a: a.__setitem__(3, a[3].astype(np.float16)),
    "R12 shape": lambda w, a: a.__setitem__(3, np.vstack([a[3], a[3][:1]])[:, :3][:3].reshape(9)),
    "R12 not finite": lambda w, a: a.__setitem__(3, np.where(np.eye(3) > 0, a[3], np.inf)),
    "t12 not finite": lambda w, a: a.__setitem__(4, np.where(np.arange(3).reshape(3, 1) == 1, np.inf, a[4])),
    "t12 a row": lambda w, a: a.__setitem__(4, a[4].reshape(1, 3)),
    "t12 float16": lambda w, a: a.__setitem__(4, a[4].astype(np.float16)),
    "s12 float32": lambda w, a: a.__setitem__(2, np.float32(a[2])),
    "s12 tiny": lambda w, a: a.__setitem__(2, 1e-320),
    "th float32": lambda w, a: a.__setitem__(5, np.float32(a[5])),
    "vpMatches12 a tuple": lambda w, a: a.__setitem__(1, tuple(a[1])),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_take_the_host_body(monkeypatch, what):
    """With a device present the public method still takes the host body, and nothing is launched."""
    m = cpu_matcher(monkeypatch, present=True)
    calls, host = [], m._sim3_host
    monkeypatch.setattr(m, "_sim3_host", lambda *a: calls.append(1) or host(*a))
    g = golden()
    w = MW.build(g)
    args = list(SC.pairs_of(w, g, 1)[0]) + [SC.TH_SIM3]
    REFUSALS[what](w, args)
    if what in ("R12 shape", "t12 a row"):   # the reference itself cannot compute with these
        assert m._sim3_prep(w.kfs[0].N, *args[:5]) is None
        return
    try:
        with np.errstate(all="ignore"):
            m.search_by_sim3(w.kfs[0], *args)
    except TypeError:
        assert what == "vpMatches12 a tuple"   # the reference writes into it
    assert len(calls) == 1


def test_zero_s12_and_a_short_list_take_the_host_body(monkeypatch):
    m = cpu_matcher(monkeypatch, present=True)
    g = golden()
    w = MW.build(g)
    kf2, vm, s12, R12, t12 = SC.pairs_of(w, g, 1)[0]
    assert m._sim3_prep(w.kfs[0].N, kf2, vm, 0, R12, t12) is None
    assert m._sim3_prep(w.kfs[0].N, kf2, vm, 0.0, R12, t12) is None
    assert m._sim3_prep(w.kfs[0].N, kf2, vm, float("nan"), R12, t12) is None
    assert m._sim3_prep(w.kfs[0].N, kf2, vm[:-1], s12, R12, t12) is None
    assert m._sim3_prep(w.kfs[0].N, kf2, vm, s12, R12, t12) is not None
    assert m._sim3_prep(w.kfs[0].N, kf2, vm, 2, R12.astype(np.float32), t12)[4]


def test_many_with_refused_elements_and_shared_lists_equals_the_loop(monkeypatch):
    """A refused keyframe in the middle and a float16 R12 take the single call at their place, the others share one
    launch; two elements that share one list take the loop."""
    launches = []
    m = oracle_device(monkeypatch, launches)
    g = golden()

    def run(many, prepare):
        w = MW.build(g)
        prs = [list(p) for p in SC.pairs_of(w, g, 4)]
        prepare(w, prs)
        f = m.search_by_sim3_many if many else SC.loop_single(m._sim3_host)
        with np.errstate(all="ignore"):
            return SC.encode(w, f(w.kfs[0], *[[p[c] for p in prs] for c in range(5)], SC.TH_SIM3))

    def refuse(w, prs):
        w.kfs[2].fx = np.float32(w.kfs[2].fx)
        prs[2][3] = prs[2][3].astype(np.float16)
    assert same(run(True, refuse), run(False, refuse))
    assert [x[1] for x in launches] == [4]   # two elements, four searches, one launch
    launches.clear()

    def share(w, prs):
        prs[1][1] = prs[0][1]
        prs[1][0] = prs[0][0]
    assert same(run(True, share), run(False, share))
    assert [x[1] for x in launches] == [2] * 4


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_new_symbols_resolve_and_abi_is_still_9():
    L = LIB.lib()
    for name in NEW:
        assert name in LIB.SIGNATURES and getattr(L, name) is not None
    assert L.orbfe_abi_version() == 9 == LIB.ORBFE_ABI_VERSION
    assert C.sizeof(LIB.Sim3Out) == 3 * C.sizeof(C.c_void_p)


def test_table_and_header_agree():
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(LIB.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_sim3_out \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in LIB.Sim3Out._fields_]
    assert int(re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1)) == 9
    assert int(re.search(r"#define ORBFE_SIM3_F64 (\d+)", hdr).group(1)) == LIB.ORBFE_SIM3_F64 == S3.SIM3_F64
    src = ROOT / "pyorbslam_amd" / "csrc" / "orbfe_fuse.hip"
    assert re.search(r"^int orbfe_sim3_search\s*\(", src.read_text(), flags=re.M)


# ---- validation: everything is refused before the first device call -------------------------------------------------

OUTS = ("best_idx", "best_dist", "status")


class HostCall:
    """orbfe_sim3_search over a small valid input (three keyframes, three searches); each test breaks one thing."""

    def __init__(self):
        c = SC.by_name("two_poses_one_target_and_idle_and_empty_keyframes")
        self.a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in SC.arrays(c).items()}
        self.n_kf, self.n_pts, self.n_srch, self.th, self.eps = 3, 1, 3, SC.TH, S3.EPS_F64
        self.o = dict(best_idx=np.full(3, -7, np.int32), best_dist=np.full(3, -7, np.int32),
                      status=np.full(3, 7, np.uint8))
        self.null = set()

    def run(self):
        p = lambda k: None if k in self.null else LIB.ptr(self.a[k])  # noqa: E731
        out = LIB.Sim3Out(**{k: None if k in self.null else v.ctypes.data for k, v in self.o.items()})
        rc = LIB.lib().orbfe_sim3_search(*[p(k) for k in S3.KF_ARRAYS], self.n_kf, p("pt_f64"), p("pt_desc"), self.n_pts,
                                         p("srch_f64"), p("srch_kf"), p("srch_off"), self.n_srch, p("item_pt"),
                                         self.th, self.eps, None if "out" in self.null else C.byref(out))
        return rc, LIB.lib().orbfe_last_error().decode()

    def untouched(self):
        return all(bool((x == (7 if k == "status" else -7)).all()) for k, x in self.o.items())


def refused(h, *words):
    rc, msg = h.run()
    assert rc == LIB.ORBFE_EINVAL and all(w in msg for w in words), (rc, msg)
    assert "ORBFE_" not in msg and h.untouched()


@pytest.mark.parametrize("name", S3.ARRAYS + ("out",) + OUTS)
def test_required_pointers(name):
    h = HostCall()
    h.null.add(name)
    refused(h, "null argument")


def test_search_checks():
    h = HostCall()
    h.a["srch_off"][0] = 1
    refused(h, "srch_off[0]", "must be 0")
    h = HostCall()
    h.a["srch_off"][1:] = [2, 1, 3]
    refused(h, "search 1", "must not decrease")
    for v in (3, -1):
        h = HostCall()
        h.a["srch_kf"][1] = v
        refused(h, "search 1", "outside the keyframes")
    for v in (1, -1):
        h = HostCall()
        h.a["item_pt"][2] = v
        refused(h, "item", "outside the point table")
    for v in (np.nan, np.inf, -np.inf):
        for col in (0, 3, 4, 13, 16, 27):
            h = HostCall()
            h.a["srch_f64"][2, col] = v
            refused(h, "search 2", "scalar", "finite")
        for col in (0, 2, 6, 7, 8):
            h = HostCall()
            h.a["pt_f64"][0, col] = v
            refused(h, "point scalar", "finite")
        for col in (20, 23, 24, 26):
            h = HostCall()
            h.a["kf_f64"][1, col] = v
            refused(h, "keyframe 1", "scalar", "finite")
        h = HostCall()
        h.th = v
        refused(h, "th and eps")
        h = HostCall()
        h.eps = v
        refused(h, "th and eps")
    h = HostCall()
    h.eps = -1e-9
    refused(h, "th and eps")
    for kw in (dict(n_kf=-1), dict(n_pts=-1), dict(n_srch=-1), dict(n_kf=65536)):
        h = HostCall()
        for k, v in kw.items():
            setattr(h, k, v)
        assert h.run()[0] == LIB.ORBFE_EINVAL and h.untouched()


def test_the_keyframe_checks_are_the_other_entries():
    for k in ("off", "cell_at", "idx_at", "lvl_off"):
        h = HostCall()
        h.a[k][0] = 1
        refused(h, "must be 0")
        h = HostCall()
        h.a[k][1], h.a[k][2] = h.a[k][2] + 1, h.a[k][2]
        refused(h, "keyframe 1", "must not decrease")
    h = HostCall()
    h.a["kf_i32"][1, 0] = 0
    refused(h, "keyframe 1", "columns and rows")
    h = HostCall()
    h.a["kf_i32"][1, 2] = 0
    refused(h, "keyframe 1", "level count")
    h = HostCall()
    h.a["cell_off"][0] = 1
    refused(h, "keyframe 0", "first cell offset")
    for v in (2, -1):
        h = HostCall()
        h.a["cell_idx"][1] = v
        refused(h, "keyframe 0", "grid entry", "outside")
    for v in (4, -1):
        h = HostCall()
        h.a["octave"][1] = v
        refused(h, "keyframe 0", "octave")
    h = HostCall()
    h.a["xy"][3, 1] = np.nan
    refused(h, "keyframe 1", "coordinate", "finite")
    h = HostCall()
    h.a["scale"][5] = np.inf
    refused(h, "keyframe 1", "level table", "finite")


def test_slots_that_are_not_read_are_not_checked_and_nothing_to_do_needs_no_device():
    """Non-finite values in the slots the mode does not read pass the validation (what follows it needs a device and
    is tests/test_gpu_sim3.py's); with no item to search the call returns before any device call."""
    h = HostCall()
    h.a["kf_f64"][:, 0:20] = np.nan
    h.a["pt_f64"][:, 3:6] = np.inf
    assert h.run()[0] != LIB.ORBFE_EINVAL
    h = HostCall()
    h.a["srch_off"][:] = 0
    assert h.run()[0] == 0 and h.untouched()
    h = HostCall()
    h.n_srch = 0
    assert h.run()[0] == 0 and h.untouched()
    h = HostCall()
    h.n_srch, h.null = 0, set(S3.ARRAYS) | {"out"}
    assert h.run()[0] == 0
