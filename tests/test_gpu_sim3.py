"""k_sim3_search on the GPU: the host entry on every placed case against the array oracle, bit for bit on all three
outputs and with guard entries around them, the reference's golden through the arrays, search_by_sim3's device path
against the golden and the host body, search_by_sim3_many against the loop and the golden from one launch, the
per-item and per-element fallbacks, concurrent callers, and the other two projection searches beside it: each
entry's own last_ms and own scratch."""
import ctypes as C
import threading

import numpy as np
import pytest

import matcher_world as MW
import scw_cases as WC
import scw_oracle as WO
import sim3_cases as SC
import sim3_oracle as S3
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]

CASES = SC.all_cases()
ORACLE = {c["name"]: SC.oracle(c) for c in CASES}  # computed once, shared, never modified
GUARD = -9


def run_host(a):
    from pyorbslam_amd.matcher import sim3_search_arrays
    r = sim3_search_arrays(*[a[k] for k in S3.ARRAYS], a["th"], a["eps"])
    return r["best_idx"], r["best_dist"], r["status"]


def assert_same(got, want, tag):
    for g, w, name in zip(got, want, ("best_idx", "best_dist", "status")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "sim3_many.npz", allow_pickle=False)


def golden_results(g, n):
    return [int(g[f"sim3_n{j}"]) for j in range(1, n + 1)], [g[f"sim3_matches{j}"] for j in range(1, n + 1)]


def same(got, want):
    return got[0] == want[0] and len(got[1]) == len(want[1]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))


def columns(prs):
    return [[p[c] for p in prs] for c in range(5)]


# ---- 1. host entry: every case, all three outputs, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_entry_matches_the_oracle(case):
    want = ORACLE[case["name"]]
    case["check"](*want)
    got = run_host(SC.arrays(case))
    assert_same(got, want, case["name"])
    assert np.flatnonzero(got[2]).tolist() == case["marked"]


@pytest.mark.parametrize("name", ["ragged_0_1_255_256_257", "zero_items", "zero_searches", "shared_points",
                                  "two_poses_one_target_and_idle_and_empty_keyframes"])
def test_guard_entries_stay_intact(name):
    """The ABI entry itself with guard entries before and behind the flat outputs."""
    from pyorbslam_amd import _lib
    a = SC.arrays(SC.by_name(name))
    n = int(a["srch_off"][-1]) if len(a["srch_off"]) else 0
    a["srch_off"] = a["srch_off"] if len(a["srch_off"]) else np.zeros(1, np.int64)
    o = dict(best_idx=np.full(n + 8, GUARD, np.int32), best_dist=np.full(n + 8, GUARD, np.int32),
             status=np.full(n + 8, 200, np.uint8))
    out = _lib.Sim3Out(**{k: v[4:].ctypes.data for k, v in o.items()})
    _lib.call("orbfe_sim3_search", *[_lib.ptr(a[k]) for k in S3.KF_ARRAYS], len(a["kf_f64"]), _lib.ptr(a["pt_f64"]),
              _lib.ptr(a["pt_desc"]), len(a["pt_f64"]), _lib.ptr(a["srch_f64"]), _lib.ptr(a["srch_kf"]),
              _lib.ptr(a["srch_off"]), len(a["srch_kf"]), _lib.ptr(a["item_pt"]), a["th"], a["eps"], C.byref(out))
    for k, (v, w) in enumerate(zip(o.values(), ORACLE[name])):
        guard = 200 if k == 2 else GUARD
        assert bool((v[:4] == guard).all()) and bool((v[4 + n:] == guard).all())
        assert np.array_equal(v[4:4 + n], w)


def test_last_ms_reports_the_launch():
    from pyorbslam_amd import _lib
    run_host(SC.arrays(CASES[0]))
    ms = C.c_float(-1)
    assert _lib.lib().orbfe_sim3_search_last_ms(C.byref(ms)) == 0 and ms.value > 0


# ---- 2. the reference's golden through the arrays ------------------------------------------------------------------
def test_golden_through_the_host_entry(golden):
    """All six pairs of the golden world in one call: the device's outputs are the oracle's bit for bit, and applying
    them gives the reference's n and vpMatches12 for every pair."""
    seen = []

    def device(a):
        got = run_host(a)
        assert_same(got, S3.search(a), "golden")
        seen.append(len(a["srch_kf"]))
        return got
    got = SC.drive(MW.build(golden), golden, lambda kf1, kfs2, vs, ss, Rs, ts, th: S3.replay(
        kf1, list(zip(kfs2, vs, ss, Rs, ts)), th, device), 6)
    assert same(got, golden_results(golden, 6)) and seen == [12]


# ---- 3. the public calls -------------------------------------------------------------------------------------------
def count_calls(monkeypatch, matcher, m):
    singles, launches = [], []
    one, arrays = m._sim3_one, matcher.sim3_search_arrays
    monkeypatch.setattr(m, "_sim3_one", lambda p, *a: singles.append(p.mnId) or one(p, *a))
    monkeypatch.setattr(matcher, "sim3_search_arrays",
                        lambda *a, **k: launches.append((len(a[0]), len(a[15]))) or arrays(*a, **k))
    return singles, launches


def test_search_by_sim3_device_path_equals_the_golden_and_the_host_body(golden, monkeypatch):
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    singles, launches = count_calls(monkeypatch, matcher, m)
    monkeypatch.setattr(m, "_sim3_host", lambda *a: pytest.fail("host body"))
    w = MW.build(golden)
    prs = SC.pairs_of(w, golden, 6)
    res = [m.search_by_sim3(w.kfs[0], *p, SC.TH_SIM3) for p in prs]
    assert same(SC.encode(w, res), golden_results(golden, 6))
    assert all(type(r) is tuple and type(r[0]) is int and r[1] is p[1] for r, p in zip(res, prs))
    assert launches == [(2, 2)] * 6
    monkeypatch.undo()
    host = SC.drive(MW.build(golden), golden, SC.loop_single(matcher.ORBMatcher()._sim3_host), 6)
    assert same(host, golden_results(golden, 6))


@pytest.mark.parametrize("n", SC.N_PAIRS)
def test_many_equal_the_loop_and_the_golden_from_one_launch(golden, monkeypatch, n):
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    loop = SC.drive(MW.build(golden), golden, SC.loop_single(m.search_by_sim3), n)
    singles, launches = count_calls(monkeypatch, matcher, m)
    w = MW.build(golden)
    prs = SC.pairs_of(w, golden, n)
    res = m.search_by_sim3_many(w.kfs[0], *columns(prs), SC.TH_SIM3)
    assert launches == [(n + 1, 2 * n)]
    assert type(res) is list and all(type(r) is tuple and type(r[0]) is int and r[1] is p[1] for r, p in zip(res, prs))
    many = SC.encode(w, res)
    assert same(many, loop) and same(many, golden_results(golden, n))


def test_forced_marginal_items_are_redone_alone(golden, monkeypatch):
    """Every tenth item comes back marked and is redone by the single-item logic: still the golden."""
    from pyorbslam_amd import _lib, matcher
    m = matcher.ORBMatcher()
    arrays = matcher.sim3_search_arrays
    forced = []

    def launch(*a, **k):
        r = arrays(*a, **k)
        r["status"][::10] |= _lib.ORBFE_FUSE_MARGINAL
        forced.append(int(np.count_nonzero(r["status"])))
        return r
    monkeypatch.setattr(matcher, "sim3_search_arrays", launch)
    one, singles = m._sim3_one, []
    monkeypatch.setattr(m, "_sim3_one", lambda *a: singles.append(1) or one(*a))
    w = MW.build(golden)
    res = m.search_by_sim3_many(w.kfs[0], *columns(SC.pairs_of(w, golden, 3)), SC.TH_SIM3)
    assert same(SC.encode(w, res), golden_results(golden, 3))
    assert len(forced) == 1 and len(singles) == forced[0] > 40


def test_genuine_marginal_item_is_redone_alone(monkeypatch):
    """A real ORBFE_FUSE_MARGINAL through both public calls: a feature exactly one radius from a point's projection,
    in both directions.  Those two items alone take the single-item logic."""
    from pyorbslam_amd import _lib, matcher
    from fuse_cases import D, pt
    n = 3
    a = dict(x=np.array([100, 303, 500], np.float32), y=np.array([100, 100, 100], np.float32),
             octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32), desc=np.stack([D(k) for k in range(n)]),
             uR=np.full(n, -1, np.float32), word=np.zeros(n, np.int32))
    th = 2.5   # level 0, scale factor 1: the radius is 2.5 px and feature 1 lies exactly that far from point 1
    for many in (False, True):
        w = MW.World()
        kfs = [MW.KeyFrame(w, j, a, np.eye(4, dtype=np.float64)) for j in range(2)]
        for kf in kfs:
            kf.Tcw = np.eye(4, dtype=np.float64)
            kf.fx = kf.fy = 64.0
            kf.cx = kf.cy = 0.0
        w.kfs = kfs
        for j, kf in enumerate(kfs):
            for i, (u, v) in enumerate(((100.5, 100.0), (300.5, 100.0), (500.25, 100.0))):
                row = pt(u, v)[0]
                row[8] = row[8] / 1.25 ** -0.5 * 1.2 ** -0.5   # the stand-in's log scale factor is log(1.2)
                p = MW.MapPoint(w, 3 * j + i, np.array(row[0:3]), D(), np.array(row[3:6]), row[6] / 0.8, row[8])
                p._pos, p._normal = p._pos.astype(np.float64), p._normal.astype(np.float64)
                w.mps.append(p)
                kf.mvpMapPoints[i] = p
        m = matcher.ORBMatcher()
        seen = []
        arrays = matcher.sim3_search_arrays
        monkeypatch.setattr(matcher, "sim3_search_arrays",
                            lambda *a, arrays=arrays, **k: seen.append(arrays(*a, **k)) or seen[-1])
        one, singles = m._sim3_one, []
        monkeypatch.setattr(m, "_sim3_one", lambda p, *a: singles.append(p.mnId) or one(p, *a))
        monkeypatch.setattr(m, "_sim3_host", lambda *a: pytest.fail("host body"))
        args = ([None] * n, 1.0, np.eye(3), np.zeros((3, 1)))
        if many:
            ret = m.search_by_sim3_many(kfs[0], [kfs[1]], *[[x] for x in args], th)[0]
        else:
            ret = m.search_by_sim3(kfs[0], kfs[1], *args, th)
        assert len(seen) == 1 and seen[0]["status"].tolist() == [0, _lib.ORBFE_FUSE_MARGINAL, 0] * 2
        assert singles == [1, 4]
        assert ret[0] == 2 and MW.encode_mps(w, ret[1]).tolist() == [3, -1, 5]
        monkeypatch.undo()


def test_many_fall_back_per_element(golden, monkeypatch):
    """A keyframe in the middle that the packer refuses and a float16 R12 take the single call at their places, a
    point with a float32 mfMaxDistance goes alone, the rest is one launch; a shared vpMatches12 list takes the loop.
    The results are the loop's."""
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()

    def world():
        w = MW.build(golden)
        w.kfs[2].fx = np.float32(w.kfs[2].fx)
        prs = [list(p) for p in SC.pairs_of(w, golden, 5)]
        prs[3][3] = prs[3][3].astype(np.float16)
        odd = next(p for i, p in enumerate(w.kfs[0].mvpMapPoints)
                   if p is not None and not p.is_bad() and not any(pr[1][i] for pr in prs))
        odd.mfMaxDistance = np.float32(odd.mfMaxDistance)
        return w, prs, odd
    w, prs, _ = world()
    with np.errstate(all="ignore"):
        loop = SC.encode(w, [m._sim3_host(w.kfs[0], *p, SC.TH_SIM3) for p in prs])
    w, prs, odd = world()
    whole, host = [], m._sim3_host
    monkeypatch.setattr(m, "_sim3_host", lambda k1, k2, *a: whole.append(k2.mnId) or host(k1, k2, *a))
    singles, launches = count_calls(monkeypatch, matcher, m)
    with np.errstate(all="ignore"):
        res = m.search_by_sim3_many(w.kfs[0], *columns(prs), SC.TH_SIM3)
    assert same(SC.encode(w, res), loop)
    assert whole == [2, 4] and launches == [(4, 6)] and singles.count(odd.mnId) == 3
    monkeypatch.undo()
    # two elements share one list: the second reads what the first wrote
    outs = []
    for many in (False, True):
        w = MW.build(golden)
        prs = [list(p) for p in SC.pairs_of(w, golden, 3)]
        prs[2][0], prs[2][1] = prs[0][0], prs[0][1]
        mm = matcher.ORBMatcher()
        launches = count_calls(monkeypatch, matcher, mm)[1]
        f = mm.search_by_sim3_many if many else SC.loop_single(mm._sim3_host)
        outs.append(SC.encode(w, f(w.kfs[0], *columns(prs), SC.TH_SIM3)))
        assert launches == ([(2, 2)] * 3 if many else [])
        monkeypatch.undo()
    assert same(outs[1], outs[0])


# ---- 4. threads and the other entries --------------------------------------------------------------------------------
def test_four_threads_get_their_own_results():
    names = ["ragged_0_1_255_256_257", "shared_points", "fuse_window_65", "depth_zero_and_either_side"]
    cases = [SC.by_name(k) for k in names]
    errors = []

    def work(case):
        try:
            a = SC.arrays(case)
            for _ in range(5):
                assert_same(run_host(a), ORACLE[case["name"]], case["name"] + " (threads)")
        except BaseException as e:  # noqa: BLE001
            errors.append((case["name"], repr(e)))
    ts = [threading.Thread(target=work, args=(c,)) for c in cases]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def run_scw(a):
    from pyorbslam_amd.matcher import scw_search_arrays
    r = scw_search_arrays(*[a[k] for k in WO.ARRAYS], a["th"], a["eps"])
    return r["best_idx"], r["best_dist"], r["status"]


def run_fuse(a):
    import fuse_oracle as FO
    from pyorbslam_amd.matcher import fuse_search_arrays
    r = fuse_search_arrays(*[a[k] for k in FO.ARRAYS], a["th"], a["eps"])
    return r["best_idx"], r["best_dist"], r["status"]


def test_each_entry_keeps_its_own_last_ms():
    """A launch of the new entry leaves the other two entries' last_ms as they were, bit for bit, and the reverse."""
    import fuse_cases as FC
    from pyorbslam_amd import _lib

    def last_ms(entry):
        ms = C.c_float(-1)
        _lib.call(entry + "_last_ms", C.byref(ms))
        return np.float32(ms.value).tobytes()
    old = next(c for c in WC.all_cases() if c["name"] == "ragged_2")
    runs = {"orbfe_sim3_search": lambda: run_host(SC.arrays(SC.by_name("shared_points"))),
            "orbfe_scw_search": lambda: run_scw(WC.arrays(old)), "orbfe_fuse_search": lambda: run_fuse(FC.arrays(old))}
    for run in runs.values():
        run()
    for first in runs:
        runs[first]()
        before = last_ms(first)
        assert np.frombuffer(before, np.float32)[0] > 0
        for other in runs:
            if other != first and "sim3" in (first + other):
                runs[other]()
                assert last_ms(first) == before, (first, other)


def test_the_entries_run_side_by_side():
    """One thread in sim3_search_arrays and one in scw_search_arrays at the same time, on different inputs: every
    call returns what the same call returned alone."""
    old = next(c for c in WC.all_cases() if c["name"] == "ragged_9")
    jobs = [(run_host, SC.arrays(SC.by_name("ragged_0_1_255_256_257"))), (run_scw, WC.arrays(old))]
    alone = [run(a) for run, a in jobs]
    errors = []

    def work(run, a, want):
        try:
            for _ in range(30):
                assert_same(run(a), want, run.__name__ + " (side by side)")
        except BaseException as e:  # noqa: BLE001
            errors.append((run.__name__, repr(e)))
    ts = [threading.Thread(target=work, args=(run, a, want)) for (run, a), want in zip(jobs, alone)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert_same(alone[0], ORACLE["ragged_0_1_255_256_257"], "ragged alone")
