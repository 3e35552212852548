"""k_ff_search on the GPU: the host entry on every placed and margin case against the array oracle, bit for bit on all
three outputs and with guard entries around them, the entry's own last_ms, the reference's golden through the arrays
from one launch, and search_by_projection_f_f_many against the golden, the six matcher_ff fixtures and the loop of
single calls, with the launches and redos it makes."""
import ctypes as C

import numpy as np
import pytest

import ff_cases as FC
import ff_margin_cases as FM
import ff_oracle as FO
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]

CASES = FC.all_cases()
ORACLE = {c["name"]: FC.oracle(c) for c in CASES}  # computed once, shared, never modified
GUARD = 99


def run_host(a):
    from pyorbslam_amd.matcher import ff_search_arrays
    return ff_search_arrays(*[a[k] for k in FO.ARRAYS], a["eps"])


def assert_same(got, want, tag):
    assert list(got) == list(FO.OUTPUTS)
    for name in FO.OUTPUTS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "ff_many.npz", allow_pickle=False)


# ---- 1. host entry: every case, all three outputs, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_entry_matches_the_oracle(case):
    want = ORACLE[case["name"]]
    case["check"](want)
    got = run_host(FC.arrays(case))
    assert_same(got, want, case["name"])
    assert np.flatnonzero(got["status"]).tolist() == case["marked"]


@pytest.mark.parametrize("name", ["ragged_0_1_255_256_257", "zero_items", "zero_searches",
                                  "two_searches_one_frame_two_ths_two_modes", "an_empty_frame_and_an_untargeted_one"])
def test_guard_entries_stay_intact(name):
    """The ABI entry itself with guard entries before and behind the flat outputs."""
    from pyorbslam_amd import _lib
    a = FC.arrays(FC.by_name(name))
    n = int(a["srch_off"][-1]) if len(a["srch_off"]) else 0
    o = {k: np.full(n + 8, GUARD, np.uint8 if k == "status" else np.int32) for k in FO.OUTPUTS}
    out = _lib.FfOut(**{k: v[4:].ctypes.data for k, v in o.items()})
    _lib.call("orbfe_ff_search", *[_lib.ptr(a[k]) for k in FO.KF_ARRAYS], len(a["kf_f64"]), _lib.ptr(a["pt_f64"]),
              _lib.ptr(a["pt_desc"]), len(a["pt_f64"]), _lib.ptr(a["srch_th"]), _lib.ptr(a["srch_mode"]),
              _lib.ptr(a["srch_kf"]), _lib.ptr(a["srch_off"]), len(a["srch_kf"]), _lib.ptr(a["item_pt"]),
              _lib.ptr(a["item_level"]), a["eps"], C.byref(out))
    for k, v in o.items():
        assert bool((v[:4] == GUARD).all()) and bool((v[4 + n:] == GUARD).all()), k
        assert np.array_equal(v[4:4 + n], ORACLE[name][k]), k


def test_last_ms_reports_the_launch():
    from pyorbslam_amd import _lib, matcher
    run_host(FC.arrays(FC.by_name("window_17")))
    ms = C.c_float(-1)
    assert _lib.lib().orbfe_ff_search_last_ms(C.byref(ms)) == 0 and ms.value > 0
    assert matcher.ff_search_last_ms() == ms.value


MARGIN_SETS = FM.all_sets()


@pytest.mark.parametrize("S", MARGIN_SETS, ids=[S.name for S in MARGIN_SETS])
def test_host_entry_matches_the_oracle_on_the_margin_ladders(S):
    a = FM.arrays(S)
    want = dict(zip(FO.OUTPUTS, FO.search(a)))
    assert want["status"][0] and want["status"][1]
    assert_same(run_host(a), want, S.name)


# ---- 2. the reference's golden through the arrays ------------------------------------------------------------------
def test_golden_through_the_host_entry(golden):
    """All six pairs in one call: the device's outputs are the oracle's bit for bit, and replaying them gives the
    reference's counts and the slots it leaves behind."""
    seen = []

    def device(a):
        got = run_host(a)
        assert_same(got, dict(zip(FO.OUTPUTS, FO.search(a))), "golden")
        seen.append((len(a["kf_f64"]), len(a["srch_kf"])))
        return tuple(got[k] for k in FO.OUTPUTS)
    jobs, objs = FC.load_world(golden)
    got = FO.replay(jobs, results=device)
    assert FC.same((got, FC.state(jobs, objs)), FC.golden_results(golden))
    assert seen == [(FC.N_PAIRS, FC.N_PAIRS)]


# ---- 3. the public call --------------------------------------------------------------------------------------------
def count_calls(monkeypatch, matcher):
    ones, launches = [], []
    one, arrays = matcher.ORBMatcher._ff_one, matcher.ff_search_arrays
    monkeypatch.setattr(matcher.ORBMatcher, "_ff_one",
                        lambda self, cur, last, i, *a: ones.append((id(cur), i)) or one(self, cur, last, i, *a))
    monkeypatch.setattr(matcher, "ff_search_arrays",
                        lambda *a, **k: launches.append((len(a[0]), len(a[18]), int(a[19][-1]))) or arrays(*a, **k))
    return ones, launches


def many(matcher, jobs):
    return matcher.ORBMatcher(0.8, True).search_by_projection_f_f_many([j[0] for j in jobs], [j[1] for j in jobs],
                                                                       [j[2] for j in jobs])


def test_many_equals_the_golden_and_the_loop_from_one_launch(golden, monkeypatch):
    """search_by_projection_f_f_many on ff_many.npz: the reference's counts and slots from exactly one launch, exactly
    the items the oracle predicts redone alone, fewer than the cap; the loop of single calls on a rebuilt world gives
    the same."""
    from pyorbslam_amd import matcher
    jobs, objs = FC.load_world(golden)
    stats = {}
    FO.replay(jobs, stats=stats)
    ones, launches = count_calls(monkeypatch, matcher)
    monkeypatch.setattr(matcher.ORBMatcher, "search_by_projection_f_f", lambda *a: pytest.fail("a single call"))
    jobs, objs = FC.load_world(golden)
    got = (many(matcher, jobs), FC.state(jobs, objs))
    assert FC.same(got, FC.golden_results(golden))
    assert launches == [(FC.N_PAIRS, FC.N_PAIRS, stats["items"])]
    assert ones == [(id(jobs[s][0]), i) for s, i in stats["redone"]] and 0 < len(ones) < FC.REDO_CAP * stats["items"]
    monkeypatch.undo()
    jobs, objs = FC.load_world(golden)
    m = matcher.ORBMatcher(0.8, True)
    loop = ([m.search_by_projection_f_f(c, x, th) for c, x, th in jobs], FC.state(jobs, objs))
    assert FC.same(loop, got)


def test_many_equals_the_six_fixtures_and_the_loop_from_one_launch(monkeypatch):
    from pyorbslam_amd import matcher
    jobs, objs, want = FC.load_fixtures()
    stats = {}
    FO.replay(jobs, stats=stats)
    ones, launches = count_calls(monkeypatch, matcher)
    monkeypatch.setattr(matcher.ORBMatcher, "search_by_projection_f_f", lambda *a: pytest.fail("a single call"))
    jobs, objs, want = FC.load_fixtures()
    got = (many(matcher, jobs), FC.state(jobs, objs))
    assert FC.same(got, ([w[0] for w in want], [w[1] for w in want]))
    assert launches == [(6, 6, stats["items"])]
    assert ones == [(id(jobs[s][0]), i) for s, i in stats["redone"]]
    monkeypatch.undo()
    jobs, objs, want = FC.load_fixtures()
    m = matcher.ORBMatcher(0.8, True)
    loop = ([m.search_by_projection_f_f(c, x, th) for c, x, th in jobs], FC.state(jobs, objs))
    assert FC.same(loop, got)


def test_genuine_marked_item_is_redone_alone(monkeypatch):
    """A real ORBFE_FUSE_MARGINAL through the public call: the identity pose, fx = fy = 64, and a feature exactly one
    radius (th 7 at octave 0) from the projection of point 1.  That item is redone alone, and the result is the loop's
    of the reference body."""
    import matcher_frames as MF
    from bow_match_cases import D
    from pyorbslam_amd import _lib, matcher
    runs = []
    for device in (True, False):
        a = dict(x=np.array([60, 120, 200], np.float32), y=np.array([100, 100, 100], np.float32),
                 octave=np.zeros(3, np.int32), angle=np.zeros(3, np.float32), desc=np.stack([D(k) for k in range(3)]),
                 uR=np.full(3, -1, np.float32))
        cur, last = FC.Frame(a, np.eye(4)), FC.Frame(a, np.eye(4))
        cur.fx = cur.fy = 64.0
        cur.cx = cur.cy = 0.0
        cur.mbf = 32.0
        last.mvpMapPoints = [MF.MP(D(), pos=np.array([[u / 64.0], [v / 64.0], [1.0]]), obs=1)
                             for u, v in ((60.5, 100.25), (113.0, 100.25), (200.25, 100.25))]
        if device:
            seen = []
            arrays = matcher.ff_search_arrays
            monkeypatch.setattr(matcher, "ff_search_arrays", lambda *a, **k: seen.append(arrays(*a, **k)) or seen[-1])
            ones, _ = count_calls(monkeypatch, matcher)
            n = matcher.ORBMatcher(0.8, False).search_by_projection_f_f_many([cur], [last], 7.0)[0]
            assert len(seen) == 1 and seen[0]["status"].tolist() == [0, _lib.ORBFE_FUSE_MARGINAL, 0]
            assert ones == [(id(cur), 1)]
            monkeypatch.undo()
        else:
            n = FO.loop(cur, last, 7.0, False)
        runs.append((n, [-1 if m is None else last.mvpMapPoints.index(m) for m in cur.mvpMapPoints]))
    assert runs[0] == runs[1] == (2, [0, -1, 2])
