"""k_fkf_search on the GPU: the host entry on every placed case against the array oracle, bit for bit on all three
outputs and with guard entries around them, the reference's golden through the arrays from one launch,
search_by_projection_f_kf_f's device path against the golden and the host body, the launches and redos it makes,
search_by_projection_f_kf_f_many against the loop and the golden from one launch, concurrent callers, and the scw and
sim3 entries beside it: each entry's own last_ms and own scratch."""
import ctypes as C
import threading

import numpy as np
import pytest

import fkf_cases as KC
import fkf_oracle as FK
import matcher_world as MW
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]

CASES = KC.all_cases()
ORACLE = {c["name"]: KC.oracle(c) for c in CASES}  # computed once, shared, never modified
GUARD = -9


def run_host(a):
    from pyorbslam_amd.matcher import fkf_search_arrays
    r = fkf_search_arrays(*[a[k] for k in FK.ARRAYS], a["th"], a["eps"])
    return r["best_idx"], r["best_dist"], r["status"]


def assert_same(got, want, tag):
    for g, w, name in zip(got, want, ("best_idx", "best_dist", "status")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "fkf.npz", allow_pickle=False)


# ---- 1. host entry: every case, all three outputs, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_entry_matches_the_oracle(case):
    want = ORACLE[case["name"]]
    case["check"](*want)
    got = run_host(KC.arrays(case))
    assert_same(got, want, case["name"])
    assert np.flatnonzero(got[2]).tolist() == case["marked"]


@pytest.mark.parametrize("name", ["ragged_0_1_255_256_257", "zero_items", "zero_searches",
                                  "four_frames_two_grids_one_empty_one_idle"])
def test_guard_entries_stay_intact(name):
    """The ABI entry itself with guard entries before and behind the flat outputs."""
    from pyorbslam_amd import _lib
    a = KC.arrays(KC.by_name(name))
    n = int(a["srch_off"][-1])
    o = dict(best_idx=np.full(n + 8, GUARD, np.int32), best_dist=np.full(n + 8, GUARD, np.int32),
             status=np.full(n + 8, 200, np.uint8))
    out = _lib.FkfOut(**{k: v[4:].ctypes.data for k, v in o.items()})
    _lib.call("orbfe_fkf_search", *[_lib.ptr(a[k]) for k in FK.KF_ARRAYS], len(a["kf_f64"]), _lib.ptr(a["pt_f64"]),
              _lib.ptr(a["pt_desc"]), len(a["pt_f64"]), _lib.ptr(a["srch_kf"]), _lib.ptr(a["srch_off"]),
              len(a["srch_kf"]), _lib.ptr(a["item_pt"]), a["th"], a["eps"], C.byref(out))
    for k, (v, w) in enumerate(zip(o.values(), ORACLE[name])):
        guard = 200 if k == 2 else GUARD
        assert bool((v[:4] == guard).all()) and bool((v[4 + n:] == guard).all())
        assert np.array_equal(v[4:4 + n], w)


def test_last_ms_reports_the_launch():
    from pyorbslam_amd import _lib
    run_host(KC.arrays(CASES[0]))
    ms = C.c_float(-1)
    assert _lib.lib().orbfe_fkf_search_last_ms(C.byref(ms)) == 0 and ms.value > 0


# ---- 2. the reference's golden through the arrays ------------------------------------------------------------------
@pytest.mark.parametrize("cfg", range(len(KC.CONFIGS)))
def test_golden_through_the_host_entry(golden, cfg):
    """All six searches of a configuration in one call: the device's outputs are the oracle's bit for bit, and
    replaying them gives the reference's n and slots for every search."""
    seen = []

    def device(a):
        got = run_host(a)
        assert_same(got, FK.search(a), "golden")
        seen.append((len(a["kf_f64"]), len(a["srch_kf"])))
        return got
    got = KC.drive(golden, KC.by_oracle(results=device), cfg)
    assert KC.same(got, KC.golden_results(golden, cfg)) and seen == [(KC.N_SEARCH, KC.N_SEARCH)]


# ---- 3. the public calls -------------------------------------------------------------------------------------------
def count_calls(monkeypatch, matcher):
    singles, launches = [], []
    one, arrays = matcher.ORBMatcher._fkf_one, matcher.fkf_search_arrays
    monkeypatch.setattr(matcher.ORBMatcher, "_fkf_one", lambda self, F, p, *a: singles.append(p) or one(self, F, p, *a))
    monkeypatch.setattr(matcher, "fkf_search_arrays",
                        lambda *a, **k: launches.append((len(a[0]), len(a[15]))) or arrays(*a, **k))
    return singles, launches


@pytest.mark.parametrize("cfg", range(len(KC.CONFIGS)))
def test_device_path_equals_the_golden_and_the_host_body(golden, monkeypatch, cfg):
    """search_by_projection_f_kf_f: the reference's n and slots from one launch per call, exactly the marked and the
    overtaken items redone alone; the host body on a rebuilt world gives the same."""
    from pyorbslam_amd import matcher
    singles, launches = count_calls(monkeypatch, matcher)
    monkeypatch.setattr(matcher.ORBMatcher, "_fkf_host", lambda *a: pytest.fail("host body"))
    stats = {}
    want = KC.drive(golden, KC.by_oracle(stats), cfg)
    got = KC.drive(golden, KC.loop_single(matcher.ORBMatcher), cfg)
    assert KC.same(got, want) and KC.same(got, KC.golden_results(golden, cfg))
    assert all(type(n) is int for n in got[0])
    assert launches == [(1, 1)] * KC.N_SEARCH and len(singles) == stats["redone"] > 0
    monkeypatch.undo()
    host = KC.drive(golden, KC.loop_single(matcher.ORBMatcher, "_fkf_host"), cfg)
    assert KC.same(host, got)


@pytest.mark.parametrize("cfg", range(len(KC.CONFIGS)))
def test_many_equal_the_loop_and_the_golden_from_one_launch(golden, monkeypatch, cfg):
    from pyorbslam_amd import matcher
    loop = KC.drive(golden, KC.loop_single(matcher.ORBMatcher), cfg)
    singles, launches = count_calls(monkeypatch, matcher)
    stats = {}
    KC.drive(golden, KC.by_oracle(stats), cfg)
    got = KC.drive(golden, KC.many(matcher.ORBMatcher), cfg)
    assert launches == [(KC.N_SEARCH, KC.N_SEARCH)] and len(singles) == stats["redone"]
    assert KC.same(got, loop) and KC.same(got, KC.golden_results(golden, cfg))


def test_genuine_marked_item_is_redone_alone(monkeypatch):
    """A real ORBFE_FUSE_MARGINAL through the public call: a feature exactly one radius from the second point's
    projection.  That item alone takes the single-item logic."""
    from fuse_cases import D, pt
    from pyorbslam_amd import _lib, matcher
    n = 3
    a = dict(x=np.array([100, 293, 490], np.float32), y=np.array([100, 100, 100], np.float32),
             octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32), desc=np.stack([D(k) for k in range(n)]),
             uR=np.full(n, -1, np.float32), word=np.zeros(n, np.int32))
    # level 0, scale factor 1: the radius is 2.5 px and feature 1 lies exactly that far from point 1.  The
    # positions are such that the stand-in's grid (cells by rounding) and the truncated window agree
    th = 2.5
    w = MW.World()
    kf = MW.KeyFrame(w, 0, a, np.eye(4))
    F = KC.Frame(w, a, np.eye(4))
    F.mTcw = F.Tcw = np.eye(4)
    F.fx = F.fy = 64.0
    F.cx = F.cy = 0.0
    for i, (u, v) in enumerate(((100.5, 100.0), (290.5, 100.0), (490.25, 100.0))):
        row = pt(u, v)[0]
        row[8] = row[8] / 1.25 ** -0.5 * 1.2 ** -0.5   # the stand-in's log scale factor is log(1.2)
        p = MW.MapPoint(w, i, np.array(row[0:3]), D(), np.array(row[3:6]), row[6] / 0.8, row[8])
        p._pos = p._pos.astype(np.float64)
        w.mps.append(p)
        kf.mvpMapPoints[i] = p
    seen = []
    arrays = matcher.fkf_search_arrays
    monkeypatch.setattr(matcher, "fkf_search_arrays", lambda *a, **k: seen.append(arrays(*a, **k)) or seen[-1])
    singles, _ = count_calls(monkeypatch, matcher)
    monkeypatch.setattr(matcher.ORBMatcher, "_fkf_host", lambda *a: pytest.fail("host body"))
    n_found = matcher.ORBMatcher(1, False).search_by_projection_f_kf_f(F, kf, set(), th, 100)
    assert len(seen) == 1 and seen[0]["status"].tolist() == [0, _lib.ORBFE_FUSE_MARGINAL, 0]
    assert [p.mnId for p in singles] == [1]
    assert n_found == 2 and MW.encode_mps(w, F.mvpMapPoints).tolist() == [0, -1, 2]


# ---- 4. threads and the other entries --------------------------------------------------------------------------------
def test_two_threads_get_their_own_results():
    cases = [KC.by_name(k) for k in ("ragged_0_1_255_256_257", "window_65")]
    errors = []

    def work(case):
        try:
            a = KC.arrays(case)
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


def test_each_entry_keeps_its_own_last_ms():
    """A launch of the new entry leaves the scw and sim3 entries' last_ms as they were, bit for bit, and the
    reverse."""
    import scw_cases as WC
    import scw_oracle as WO
    import sim3_cases as SC
    import sim3_oracle as S3
    from pyorbslam_amd import _lib, matcher

    def last_ms(entry):
        ms = C.c_float(-1)
        _lib.call(entry + "_last_ms", C.byref(ms))
        return np.float32(ms.value).tobytes()
    scw = WC.arrays(next(c for c in WC.all_cases() if c["name"] == "ragged_2"))
    sim3 = SC.arrays(SC.by_name("shared_points"))
    runs = {"orbfe_fkf_search": lambda: run_host(KC.arrays(KC.by_name("window_65"))),
            "orbfe_scw_search": lambda: matcher.scw_search_arrays(*[scw[k] for k in WO.ARRAYS], scw["th"], scw["eps"]),
            "orbfe_sim3_search": lambda: matcher.sim3_search_arrays(*[sim3[k] for k in S3.ARRAYS], sim3["th"],
                                                                    sim3["eps"])}
    for run in runs.values():
        run()
    for first in runs:
        runs[first]()
        before = last_ms(first)
        assert np.frombuffer(before, np.float32)[0] > 0
        for other in runs:
            if other != first and "fkf" in (first + other):
                runs[other]()
                assert last_ms(first) == before, (first, other)
