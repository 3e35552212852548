"""k_scw_search on the GPU: the host entry on every placed case against the array oracle, bit for bit on all three
outputs and with guard rows around them, the reference's golden through the arrays, fuse_kf_scw_mp_many against loops
of fuse_kf_scw_mp and against the golden, search_by_projection_ckf_scw_mp's device path against the golden and the
host body, the per-item fallbacks of both, concurrent callers, and orbfe_fuse_search beside it: each entry's own last_ms
and own scratch."""
import ctypes as C
import threading

import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as FO
import matcher_world as MW
import scw_cases as SC
import scw_oracle as SO
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]

CASES = SC.all_cases()
ORACLE = {c["name"]: SC.oracle(c) for c in CASES}  # computed once, shared, never modified
GUARD = -9


def run_host(a):
    from pyorbslam_amd.matcher import scw_search_arrays
    r = scw_search_arrays(*[a[k] for k in SO.ARRAYS], a["th"], a["eps"])
    return r["best_idx"], r["best_dist"], r["status"]


def assert_same(got, want, tag):
    for g, w, name in zip(got, want, ("best_idx", "best_dist", "status")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "scw_many.npz", allow_pickle=False)


# ---- 1. host entry: every case, all three outputs, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_entry_matches_the_oracle(case):
    from pyorbslam_amd import _lib
    want = ORACLE[case["name"]]
    case["check"](*want)
    got = run_host(SC.arrays(case))
    assert_same(got, want, case["name"])
    if case["name"] == "marginal":
        assert got[2].tolist() == [[0, _lib.ORBFE_FUSE_MARGINAL, 0]]
    else:
        assert not got[2].any()


def test_the_bf_slot_is_not_read():
    case = next(c for c in CASES if c["name"] == "ragged_9")
    a = SC.arrays(case)
    a["kf_f64"] = a["kf_f64"].copy()
    a["kf_f64"][:, 4] = [np.nan, np.inf, -1e300, 0.0, 1.0, np.nan, 7.0, -np.inf, 3.0]
    assert_same(run_host(a), ORACLE["ragged_9"], "bf")


@pytest.mark.parametrize("name", ["ragged_9", f"points_{SC.CHUNK + 1}", "window_17", "keyframe_without_features",
                                  "blocked_ragged"])
def test_guard_rows_stay_intact(name):
    """The ABI entry itself with guard rows before and behind every output and guard entries behind every row."""
    from pyorbslam_amd import _lib
    case = next(c for c in CASES if c["name"] == name)
    a = SC.arrays(case)
    K, P = len(a["kf_f64"]), len(a["pt_f64"])
    stride = P + 3
    o = dict(best_idx=np.full((K + 2, stride), GUARD, np.int32), best_dist=np.full((K + 2, stride), GUARD, np.int32),
             status=np.full((K + 2, stride), 200, np.uint8))
    out = _lib.ScwOut(**{k: v[1:].ctypes.data for k, v in o.items()})
    _lib.call("orbfe_scw_search", *[_lib.ptr(a[k]) for k in SO.ARRAYS[:13]], K, _lib.ptr(a["pt_f64"]),
              _lib.ptr(a["pt_desc"]), P, a["th"], a["eps"], C.byref(out), stride)
    for k, (v, w) in enumerate(zip(o.values(), ORACLE[name])):
        guard = 200 if k == 2 else GUARD
        assert bool((v[0] == guard).all()) and bool((v[K + 1] == guard).all()) and bool((v[1:K + 1, P:] == guard).all())
        assert np.array_equal(v[1:K + 1, :P], w)


def test_last_ms_reports_the_launch():
    from pyorbslam_amd import _lib
    run_host(SC.arrays(CASES[0]))
    ms = C.c_float(-1)
    assert _lib.lib().orbfe_scw_search_last_ms(C.byref(ms)) == 0 and ms.value > 0


# ---- 2. the reference's golden through the arrays ------------------------------------------------------------------
def test_golden_through_the_host_entry(golden):
    """Both runs of the golden world: the device's outputs are the oracle's bit for bit, and replaying them gives
    the reference's returns, vpReplacePoint / vpMatched, log, slots, bad flags and descriptors."""
    seen = []

    def device(a):
        got = run_host(a)
        assert_same(got, SO.search(a), "golden")
        seen.append(got[0].shape)
        return got
    w = MW.build(golden)
    res = SC.drive_fuse(w, golden, lambda kfs, S, pts, th, after: SO.replay_fuse(kfs, S, pts, th, after, device), 6)
    SC.assert_state(SC.fuse_state(w, res), SC.golden_state(golden, 6))
    n, vm = SC.drive_ckf(MW.build(golden), golden, lambda kf, S, pts, m, th: SO.replay_ckf(kf, S, pts, m, th, device))
    assert n == int(golden["ckf_n"]) and np.array_equal(vm, golden["ckf_matched"])
    assert len(seen) == 2 and seen[0][0] == 6 and seen[1][0] == 1


# ---- 3. the _many drop-in --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,prefix", [(1, "n"), (3, "n"), (6, "n"), (6, "p")])
def test_many_equal_a_loop_and_the_golden(golden, n, prefix):
    """search_and_fuse over n keyframes on fresh builds: the returns, the vpReplacePoint lists, the log, the slots,
    the bad flags and the descriptors of the many call are those of the loop of fuse_kf_scw_mp and those the
    reference left in the golden; prefix p: after=None against the loop without the replace."""
    from pyorbslam_amd.matcher import ORBMatcher
    m = ORBMatcher()
    after = prefix == "n"
    w1, w2 = MW.build(golden), MW.build(golden)
    loop = SC.fuse_state(w1, SC.drive_fuse(w1, golden, SC.loop_fuse(m.fuse_kf_scw_mp), n, after))
    res = SC.drive_fuse(w2, golden, m.fuse_kf_scw_mp_many, n, after)
    many = SC.fuse_state(w2, res)
    SC.assert_state(many, loop, "many against the loop")
    SC.assert_state(many, SC.golden_state(golden, n, prefix), "many against the golden")
    assert all(type(r) is tuple and type(r[0]) is int and type(r[1]) is list for r in res)


def count_calls(monkeypatch, matcher, m):
    singles, launches = [], []
    one, arrays = m._scw_one, matcher.scw_search_arrays
    monkeypatch.setattr(m, "_scw_one",
                        lambda kf, p, *a: singles.append((kf.mnId, p.mnId)) or one(kf, p, *a))
    monkeypatch.setattr(matcher, "scw_search_arrays",
                        lambda *a, **k: launches.append((len(a[0]), len(a[13]))) or arrays(*a, **k))
    return singles, launches


def test_many_fall_back_per_element(golden, monkeypatch):
    """A keyframe in the middle that the packer refuses and one whose Scw is float16 take fuse_kf_scw_mp whole at
    their places; a point that the arrays cannot express goes alone in every other keyframe; the rest is one
    launch."""
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    states = []
    for many in (False, True):
        w = MW.build(golden)
        w.kfs[2].fx = np.float32(w.kfs[2].fx)
        S = SC.scws(golden, 5)
        S[3] = S[3].astype(np.float16)
        pts = SC.loop_points(w)
        odd = next(p for p in pts if not p.is_bad() and not any(p.is_in_key_frame(kf) for kf in w.kfs[1:6]))
        odd.mfMaxDistance = np.float32(odd.mfMaxDistance)
        if many:
            whole = []
            single = m.fuse_kf_scw_mp
            monkeypatch.setattr(m, "fuse_kf_scw_mp", lambda kf, *a: whole.append(kf.mnId) or single(kf, *a))
            singles, launches = count_calls(monkeypatch, matcher, m)
            n_sent = sum(1 for p in pts if not p.is_bad()) - 1
            res = m.fuse_kf_scw_mp_many(w.kfs[1:6], S, pts, SC.TH_FUSE, SC.replacer(pts))
            assert whole == [2, 4] and launches == [(3, n_sent)]
            assert {k for k, i in singles if i == odd.mnId} <= {1, 3, 5} and any(i == odd.mnId for _, i in singles)
        else:
            res = SC.loop_fuse(m.fuse_kf_scw_mp)(w.kfs[1:6], S, pts, SC.TH_FUSE, SC.replacer(pts))
        states.append(SC.fuse_state(w, res))
    SC.assert_state(states[1], states[0])
    assert int(states[0]["ret"].sum()) > 0


def test_forced_marginal_items_are_redone_alone(golden, monkeypatch):
    """Every tenth item comes back marked: those that the replay reaches are redone by the single-item logic, in
    both searches, and the results are still the golden's."""
    from pyorbslam_amd import _lib, matcher
    m = matcher.ORBMatcher()
    arrays = matcher.scw_search_arrays
    forced = []

    def launch(*a, **k):
        r = arrays(*a, **k)
        r["status"].reshape(-1)[::10] |= _lib.ORBFE_FUSE_MARGINAL
        forced.append(int(np.count_nonzero(r["status"])))
        return r
    monkeypatch.setattr(matcher, "scw_search_arrays", launch)
    one, singles = m._scw_one, []
    monkeypatch.setattr(m, "_scw_one", lambda *a: singles.append(a[-1] is not None and len(a) == 7) or one(*a))
    w = MW.build(golden)
    many = SC.fuse_state(w, SC.drive_fuse(w, golden, m.fuse_kf_scw_mp_many, 3))
    SC.assert_state(many, SC.golden_state(golden, 3))
    assert len(forced) == 1 and forced[0] > 50 and len(singles) > 20
    n_fuse = len(singles)
    n, vm = SC.drive_ckf(MW.build(golden), golden, m.search_by_projection_ckf_scw_mp)
    assert n == int(golden["ckf_n"]) and np.array_equal(vm, golden["ckf_matched"])
    assert len(forced) == 2 and len(singles) - n_fuse >= forced[1] > 10 and all(singles[n_fuse:])


def test_genuine_marginal_item_is_redone_alone(monkeypatch):
    """A real ORBFE_FUSE_MARGINAL through both drop-ins: a feature exactly one radius from a point's projection.
    That item alone takes the single-item logic."""
    from pyorbslam_amd import _lib, matcher
    from fuse_cases import D, pt
    n = 3
    a = dict(x=np.array([100, 303, 500], np.float32), y=np.array([100, 100, 100], np.float32),
             octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32), desc=np.stack([D(k) for k in range(n)]),
             uR=np.full(n, -1, np.float32), word=np.zeros(n, np.int32))
    th = 2.5   # level 0, scale factor 1: the radius is 2.5 px and feature 1 lies exactly that far from point 1
    for ckf in (False, True):
        w = MW.World()
        kfs = [MW.KeyFrame(w, j, a, np.eye(4, dtype=np.float64)) for j in range(2)]
        for kf in kfs:
            kf.Tcw = np.eye(4, dtype=np.float64)
            kf.fx = kf.fy = 64.0
            kf.cx = kf.cy = 0.0
        w.kfs = kfs
        for i, (u, v) in enumerate(((100.5, 100.0), (300.5, 100.0), (500.25, 100.0))):
            row = pt(u, v)[0]
            row[8] = row[8] / 1.25 ** -0.5 * 1.2 ** -0.5   # the stand-in's log scale factor is log(1.2)
            p = MW.MapPoint(w, i, np.array(row[0:3]), D(), np.array(row[3:6]), row[6] / 0.8, row[8])
            p._pos, p._normal = p._pos.astype(np.float64), p._normal.astype(np.float64)
            w.mps.append(p)
        m = matcher.ORBMatcher()
        seen = []
        arrays = matcher.scw_search_arrays
        monkeypatch.setattr(matcher, "scw_search_arrays", lambda *a, arrays=arrays, **k: seen.append(arrays(*a, **k)) or seen[-1])
        one, singles = m._scw_one, []
        monkeypatch.setattr(m, "_scw_one", lambda kf, p, *a: singles.append((kf.mnId, p.mnId)) or one(kf, p, *a))
        S = [np.eye(4), 2.0 * np.eye(4)]
        if ckf:
            ret = m.search_by_projection_ckf_scw_mp(kfs[1], S[1], w.mps, [None] * n, th)
            assert len(seen) == 1 and seen[0]["status"].tolist() == [[0, _lib.ORBFE_FUSE_MARGINAL, 0]]
            assert singles == [(1, 1)]
            assert ret[0] == 2 and MW.encode_mps(w, ret[1]).tolist() == [0, -1, 2]
        else:
            ret = m.fuse_kf_scw_mp_many(kfs, S, w.mps, th)
            assert len(seen) == 1 and seen[0]["status"].tolist() == [[0, _lib.ORBFE_FUSE_MARGINAL, 0]] * 2
            assert singles == [(0, 1), (1, 1)]
            assert [r[0] for r in ret] == [2, 2]
        monkeypatch.undo()


# ---- 4. the ckf device path --------------------------------------------------------------------------------------------
def test_ckf_device_path_equals_the_golden_and_the_host_body(golden, monkeypatch):
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    singles, launches = count_calls(monkeypatch, matcher, m)
    monkeypatch.setattr(m, "_ckf_host", lambda *a: pytest.fail("host body"))
    n, vm = SC.drive_ckf(MW.build(golden), golden, m.search_by_projection_ckf_scw_mp)
    assert n == int(golden["ckf_n"]) and np.array_equal(vm, golden["ckf_matched"])
    assert len(launches) == 1 and launches[0][0] == 1
    # the items whose candidate an earlier point of the call took are redone alone, and nothing else is
    stats = {}
    SC.drive_ckf(MW.build(golden), golden, lambda kf, S, pts, v, th: SO.replay_ckf(kf, S, pts, v, th, stats=stats))
    assert stats["marginal"] == 0 and len(singles) == stats["taken"] > 0
    monkeypatch.undo()
    n2, vm2 = SC.drive_ckf(MW.build(golden), golden, matcher.ORBMatcher()._ckf_host)
    assert n2 == n and np.array_equal(vm2, vm)


def test_ckf_inexpressible_point_goes_alone(golden, monkeypatch):
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    want = np.asarray(golden["ckf_matched"])
    pre = np.asarray(golden["ckf_pre"])
    w = MW.build(golden)
    odd = w.mps[int(next(i for i, p in zip(want, pre) if i >= 0 and p < 0))]   # a point the call matches
    odd.mfMaxDistance = np.float32(odd.mfMaxDistance)
    singles, launches = count_calls(monkeypatch, matcher, m)
    n, vm = SC.drive_ckf(w, golden, m.search_by_projection_ckf_scw_mp)
    assert (1, odd.mnId) in singles and len(launches) == 1
    w2 = MW.build(golden)
    w2.mps[odd.mnId].mfMaxDistance = np.float32(w2.mps[odd.mnId].mfMaxDistance)
    n2, vm2 = SC.drive_ckf(w2, golden, matcher.ORBMatcher()._ckf_host)
    assert n == n2 and np.array_equal(vm, vm2)


# ---- 5. four threads ------------------------------------------------------------------------------------------------
def test_four_threads_get_their_own_results():
    names = ["ragged_9", f"points_{SC.CHUNK + 1}", "blocked_ragged", "poses_float32"]
    cases = [next(c for c in CASES if c["name"] == k) for k in names]
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


# ---- 6. the two entries share their code, not their state --------------------------------------------------------------
def run_fuse(a):
    from pyorbslam_amd.matcher import fuse_search_arrays
    r = fuse_search_arrays(*[a[k] for k in FO.ARRAYS], a["th"], a["eps"])
    return r["best_idx"], r["best_dist"], r["status"]


def fuse_arrays(name, n_pts=None):
    """The fuse entry's arrays of a case (its points cut to n_pts), and the scw entry's of the same case."""
    case = dict(next(c for c in CASES if c["name"] == name))
    if n_pts is not None:
        case["pt_f64"], case["pt_desc"] = case["pt_f64"][:n_pts].copy(), case["pt_desc"][:n_pts].copy()
    return FC.arrays(case), SC.arrays(case)


def test_each_entry_keeps_its_own_last_ms():
    """A launch of one entry leaves the other's last_ms as it was, bit for bit, in both directions."""
    from pyorbslam_amd import _lib

    def last_ms(entry):
        ms = C.c_float(-1)
        _lib.call(entry + "_last_ms", C.byref(ms))
        return np.float32(ms.value).tobytes()
    fuse, scw = fuse_arrays("ragged_2", 3)
    for first, run_first, run_other, a, b in (("orbfe_fuse_search", run_fuse, run_host, fuse, scw),
                                              ("orbfe_scw_search", run_host, run_fuse, scw, fuse)):
        run_first(a)
        before = last_ms(first)
        assert np.frombuffer(before, np.float32)[0] > 0
        run_other(b)
        assert last_ms(first) == before, first


def test_the_entries_run_side_by_side():
    """One thread in fuse_search_arrays and one in scw_search_arrays at the same time, on different inputs: every
    call returns what the same call returned alone."""
    jobs = [(run_fuse, fuse_arrays("ragged_2")[0]), (run_host, fuse_arrays("ragged_9")[1])]
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
    assert_same(alone[1], ORACLE["ragged_9"], "ragged_9 alone")
