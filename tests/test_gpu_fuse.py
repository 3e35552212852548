"""k_fuse_search on the GPU: the host entry on every crafted case against the array oracle, bit for bit on all three
outputs and with guard rows around them, the reference's golden through the arrays, fuse_pkf_mp_many against loops
of fuse_pkf_mp and against the golden, its per-item fallbacks, and concurrent callers."""
import ctypes as C
import threading

import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = FC.all_cases()
ORACLE = {c["name"]: FC.oracle(c) for c in CASES}  # computed once, shared, never modified
GUARD = -9


def run_host(a):
    from pyorbslam_amd.matcher import fuse_search_arrays
    r = fuse_search_arrays(*[a[k] for k in O.ARRAYS], a["th"], a["eps"])
    return r["best_idx"], r["best_dist"], r["status"]


def assert_same(got, want, tag):
    for g, w, name in zip(got, want, ("best_idx", "best_dist", "status")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "fuse_many.npz", allow_pickle=False)


# ---- 1. host entry: every case, all three outputs, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_entry_matches_the_oracle(case):
    from pyorbslam_amd import _lib
    want = ORACLE[case["name"]]
    case["check"](*want)
    got = run_host(FC.arrays(case))
    assert_same(got, want, case["name"])
    if case["name"] == "marginal":
        assert got[2].tolist() == [[0, _lib.ORBFE_FUSE_MARGINAL, 0]]
    else:
        assert not got[2].any()


@pytest.mark.parametrize("name", ["ragged_9", f"points_{FC.CHUNK + 1}", "window_129", "keyframe_without_features"])
def test_guard_rows_stay_intact(name):
    """The ABI entry itself with guard rows before and behind every output and guard entries behind every row."""
    from pyorbslam_amd import _lib
    case = next(c for c in CASES if c["name"] == name)
    a = FC.arrays(case)
    K, P = len(a["kf_f64"]), len(a["pt_f64"])
    stride = P + 3
    o = dict(best_idx=np.full((K + 2, stride), GUARD, np.int32), best_dist=np.full((K + 2, stride), GUARD, np.int32),
             status=np.full((K + 2, stride), 200, np.uint8))
    out = _lib.FuseOut(**{k: v[1:].ctypes.data for k, v in o.items()})
    _lib.call("orbfe_fuse_search", *[_lib.ptr(a[k]) for k in O.ARRAYS[:14]], K, _lib.ptr(a["pt_f64"]),
              _lib.ptr(a["pt_desc"]), P, a["th"], a["eps"], C.byref(out), stride)
    for k, (v, w) in enumerate(zip(o.values(), ORACLE[name])):
        guard = 200 if k == 2 else GUARD
        assert bool((v[0] == guard).all()) and bool((v[K + 1] == guard).all()) and bool((v[1:K + 1, P:] == guard).all())
        assert np.array_equal(v[1:K + 1, :P], w)


def test_last_ms_reports_the_launch():
    from pyorbslam_amd import _lib
    run_host(FC.arrays(CASES[0]))
    ms = C.c_float(-1)
    assert _lib.lib().orbfe_fuse_search_last_ms(C.byref(ms)) == 0 and ms.value > 0


# ---- 2. the reference's golden through the arrays ------------------------------------------------------------------
def test_golden_through_the_host_entry(golden):
    """Both calls of the golden world (fresh, before any side effect): the device's outputs are the oracle's bit for
    bit, and replaying them gives the reference's returns, log, slots, bad flags and descriptors."""
    import matcher_world as MW
    w = MW.build(golden)
    pts = [p for p in w.kfs[0].get_map_point_matches() if p is not None]
    for kfs, points in ((w.kfs[1:], pts), ([w.kfs[0]], FC.pooled_points(w.kfs[1:]))):
        a = O.pack(kfs, points, FC.TH)
        assert_same(run_host(a), O.search(a), "golden")

    def fuse(kfs, points, th):
        sent = [p for p in points if p is not None]
        return O.replay(kfs, points, th, results=run_host(O.pack(kfs, sent, th)))
    w = FC.load_world(golden)
    FC.assert_state(FC.world_state(w, FC.drive(w, fuse, 6)), FC.golden_state(golden, 6))


# ---- 3. the _many drop-in --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FC.N_NEIGH)
def test_many_equal_a_loop_and_the_golden(golden, n):
    """Both calls of search_in_neighbors (n neighbours, then the pooled points into the current keyframe) on fresh
    builds: the returns, the log, the slots, the bad flags and the descriptors of the many call are those of the loop
    of fuse_pkf_mp and those the reference left in the golden."""
    from pyorbslam_amd.matcher import ORBMatcher
    m = ORBMatcher()
    w1, w2 = FC.load_world(golden), FC.load_world(golden)
    loop = FC.world_state(w1, FC.drive(w1, lambda kfs, pts, th: [m.fuse_pkf_mp(kf, pts, th) for kf in kfs], n))
    many = FC.world_state(w2, FC.drive(w2, m.fuse_pkf_mp_many, n))
    FC.assert_state(many, loop, "many against the loop")
    FC.assert_state(many, FC.golden_state(golden, n), "many against the golden")
    assert all(type(x) is int for x in FC.drive(FC.load_world(golden), m.fuse_pkf_mp_many, 1))


def count_calls(monkeypatch, matcher, m):
    singles, launches = [], []
    one, arrays = m._fuse_one, matcher.fuse_search_arrays
    monkeypatch.setattr(m, "_fuse_one", lambda kf, p, th, K: singles.append((kf.mnId, p.mnId)) or one(kf, p, th, K))
    monkeypatch.setattr(matcher, "fuse_search_arrays",
                        lambda *a, **k: launches.append((len(a[0]), len(a[14]))) or arrays(*a, **k))
    return singles, launches


def test_many_fall_back_per_element(golden, monkeypatch):
    """A keyframe in the middle that the packer refuses takes fuse_pkf_mp whole at its place; a point that the arrays
    cannot express goes alone in every keyframe; the rest is one launch."""
    from pyorbslam_amd import matcher
    m = matcher.ORBMatcher()
    states = []
    for many in (False, True):
        w = FC.load_world(golden)
        w.kfs[2].fx = np.float32(w.kfs[2].fx)
        pts = w.kfs[0].get_map_point_matches()
        odd = next(p for p in pts if p is not None and not p.is_bad()
                   and not any(p.is_in_key_frame(kf) for kf in w.kfs[1:5]))
        odd.mfMaxDistance = np.float32(odd.mfMaxDistance)
        if many:
            whole = []
            single = m.fuse_pkf_mp
            monkeypatch.setattr(m, "fuse_pkf_mp", lambda kf, p, th: whole.append(kf.mnId) or single(kf, p, th))
            singles, launches = count_calls(monkeypatch, matcher, m)
            n_sent = sum(1 for p in pts if p is not None and not p.is_bad()) - 1
            ret = m.fuse_pkf_mp_many(w.kfs[1:5], pts, FC.TH)
            assert whole == [2] and launches == [(3, n_sent)]
            assert {k for k, i in singles if i == odd.mnId} <= {1, 3, 4} and any(i == odd.mnId for _, i in singles)
        else:
            ret = [m.fuse_pkf_mp(kf, pts, FC.TH) for kf in w.kfs[1:5]]
        states.append(FC.world_state(w, ret))
    FC.assert_state(states[1], states[0])
    assert int(states[0]["ret"].sum()) > 0


def test_forced_marginal_items_are_redone_alone(golden, monkeypatch):
    """Every tenth item comes back marked: exactly those that the replay reaches are redone by the single-item
    logic, and the results are still the loop's."""
    from pyorbslam_amd import _lib, matcher
    m = matcher.ORBMatcher()
    w1, w2 = FC.load_world(golden), FC.load_world(golden)
    pts1, pts2 = w1.kfs[0].get_map_point_matches(), w2.kfs[0].get_map_point_matches()
    loop = FC.world_state(w1, [m.fuse_pkf_mp(kf, pts1, FC.TH) for kf in w1.kfs[1:4]])
    arrays = matcher.fuse_search_arrays
    forced = []

    def launch(*a, **k):
        r = arrays(*a, **k)
        r["status"].reshape(-1)[::10] |= _lib.ORBFE_FUSE_MARGINAL
        forced.append(int(np.count_nonzero(r["status"])))
        return r
    monkeypatch.setattr(matcher, "fuse_search_arrays", launch)
    one, singles = m._fuse_one, []
    monkeypatch.setattr(m, "_fuse_one", lambda kf, p, th, K: singles.append(1) or one(kf, p, th, K))
    many = FC.world_state(w2, m.fuse_pkf_mp_many(w2.kfs[1:4], pts2, FC.TH))
    FC.assert_state(many, loop)
    assert len(forced) == 1 and forced[0] > 50 and len(singles) > 20


def test_genuine_marginal_item_is_redone_alone(monkeypatch):
    """A real ORBFE_FUSE_MARGINAL through the drop-in: a keyframe whose level-0 inverse sigma square is 5.99 and a
    feature exactly one pixel from a point's projection.  That item alone takes the single-item logic."""
    import matcher_world as MW
    from pyorbslam_amd import _lib, matcher
    n = 3
    a = dict(x=np.array([100, 300, 500], np.float32), y=np.array([100, 100.5, 100], np.float32),
             octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32), desc=np.stack([FC.D(k) for k in range(n)]),
             uR=np.full(n, -1, np.float32), word=np.zeros(n, np.int32))
    states = []
    for many in (False, True):
        w = MW.World()
        kfs = [MW.KeyFrame(w, j, a, np.eye(4, dtype=np.float64)) for j in range(2)]
        for kf in kfs:
            kf.Tcw = np.eye(4, dtype=np.float64)
            kf.fx = kf.fy = 64.0
            kf.cx = kf.cy = 0.0
        kfs[1].mvInvLevelSigma2 = [5.99] + list(MW.INV_SIG2[1:])
        for i, (u, v) in enumerate(((100.5, 100.0), (300.0, 101.5), (500.25, 100.0))):
            row = FC.pt(u, v, q=-0.5 / 1.0)[0]
            row[8] = row[8] / 1.25 ** -0.5 * 1.2 ** -0.5   # the stand-in's log scale factor is log(1.2)
            p = MW.MapPoint(w, i, np.array(row[0:3]), FC.D(), np.array(row[3:6]), row[6] / 0.8, row[8])
            p._pos, p._normal = p._pos.astype(np.float64), p._normal.astype(np.float64)
            w.mps.append(p)
        m = matcher.ORBMatcher()
        if many:
            seen = []
            arrays = matcher.fuse_search_arrays
            monkeypatch.setattr(matcher, "fuse_search_arrays", lambda *a, **k: seen.append(arrays(*a, **k)) or seen[-1])
            one, singles = m._fuse_one, []
            monkeypatch.setattr(m, "_fuse_one", lambda kf, p, th, K: singles.append((kf.mnId, p.mnId)) or one(kf, p, th, K))
            ret = m.fuse_pkf_mp_many(kfs, w.mps, FC.TH)
            assert len(seen) == 1 and seen[0]["status"].tolist() == [[0, 0, 0], [0, _lib.ORBFE_FUSE_MARGINAL, 0]]
            assert singles == [(1, 1)]
        else:
            ret = [m.fuse_pkf_mp(kf, w.mps, FC.TH) for kf in kfs]
        w.kfs = kfs
        states.append(FC.world_state(w, ret))
    FC.assert_state(states[1], states[0])
    assert states[0]["ret"].tolist() == [3, 3]


# ---- 4. four threads ------------------------------------------------------------------------------------------------
def test_four_threads_get_their_own_results():
    names = ["ragged_9", f"points_{FC.CHUNK + 1}", "window_129", "poses_float32"]
    cases = [next(c for c in CASES if c["name"] == k) for k in names]
    errors = []

    def work(case):
        try:
            a = FC.arrays(case)
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
