"""k_local_search on the GPU: the host entry on every placed case against the array oracle, bit for bit on all seven
outputs and with guard entries around them, the reference's golden through the arrays from one launch,
search_local_points' device path against the golden and the loop, the launches and redos it makes,
search_local_points_many against the loop and the golden from one launch, the entry's own last_ms, and frames 1-3 of
the C3 tracking loop through the GPU extractor and search_local_points against that golden's record."""
import ctypes as C

import numpy as np
import pytest

import local_search_cases as LC
import local_search_oracle as LO
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]

CASES = LC.all_cases()
ORACLE = {c["name"]: LC.oracle(c) for c in CASES}  # computed once, shared, never modified
GUARD = 99
REDO_CAP = 0.05


def run_host(a):
    from pyorbslam_amd.matcher import local_search_arrays
    return local_search_arrays(*[a[k] for k in LO.ARRAYS], a["th"], a["th_on"], a["eps"])


def assert_same(got, want, tag):
    assert list(got) == list(LO.OUTPUTS)
    for name in LO.OUTPUTS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "local_search.npz", allow_pickle=False)


# ---- 1. host entry: every case, all seven outputs, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_entry_matches_the_oracle(case):
    want = ORACLE[case["name"]]
    case["check"](want)
    got = run_host(LC.arrays(case))
    assert_same(got, want, case["name"])
    assert np.flatnonzero(got["status"]).tolist() == case["marked"]


@pytest.mark.parametrize("name", ["ragged_0_1_255_256_257", "zero_items", "zero_searches",
                                  "two_limits_an_empty_frame_and_an_idle_one", "window_17"])
def test_guard_entries_stay_intact(name):
    """The ABI entry itself with guard entries before and behind the flat outputs."""
    from pyorbslam_amd import _lib
    a = LC.arrays(LC.by_name(name))
    n = int(a["srch_off"][-1]) if len(a["srch_off"]) else 0
    o = {k: np.full(n + 8, GUARD, np.uint8 if k in ("in_view", "status") else np.int32) for k in LO.OUTPUTS}
    out = _lib.LocalOut(**{k: v[4:].ctypes.data for k, v in o.items()})
    _lib.call("orbfe_local_search", *[_lib.ptr(a[k]) for k in LO.KF_ARRAYS], len(a["kf_f64"]), _lib.ptr(a["pt_f64"]),
              _lib.ptr(a["pt_desc"]), len(a["pt_f64"]), _lib.ptr(a["srch_limit"]), _lib.ptr(a["srch_kf"]),
              _lib.ptr(a["srch_off"]), len(a["srch_kf"]), _lib.ptr(a["item_pt"]), a["th"], int(a["th_on"]), a["eps"],
              C.byref(out))
    for k, v in o.items():
        assert bool((v[:4] == GUARD).all()) and bool((v[4 + n:] == GUARD).all()), k
        assert np.array_equal(v[4:4 + n], ORACLE[name][k]), k


def test_last_ms_reports_the_launch():
    from pyorbslam_amd import _lib, matcher
    run_host(LC.arrays(LC.by_name("window_17")))
    ms = C.c_float(-1)
    assert _lib.lib().orbfe_local_search_last_ms(C.byref(ms)) == 0 and ms.value > 0
    assert matcher.local_search_last_ms() == ms.value


# ---- 2. the reference's golden through the arrays ------------------------------------------------------------------
@pytest.mark.parametrize("cfg", range(len(LC.CONFIGS)))
def test_golden_through_the_host_entry(golden, cfg):
    """Both frames of a configuration in one call: the device's outputs are the oracle's bit for bit, and replaying
    them gives the reference's results and everything the reference leaves behind."""
    seen = []

    def device(a):
        got = run_host(a)
        assert_same(got, dict(zip(LO.OUTPUTS, LO.search(a))), "golden")
        seen.append((len(a["kf_f64"]), len(a["srch_kf"])))
        return tuple(got[k] for k in LO.OUTPUTS)
    got = LC.drive(golden, LC.by_oracle(results=device), cfg)
    want = LC.golden_results(golden, cfg)
    assert LC.same(got, want), LC.diff(got, want)
    assert seen == [(LC.N_FRAMES, LC.N_FRAMES)]


# ---- 3. the public calls -------------------------------------------------------------------------------------------
def count_calls(monkeypatch, matcher):
    singles, launches = [], []
    one, arrays = matcher.ORBMatcher._fp_one, matcher.local_search_arrays
    monkeypatch.setattr(matcher.ORBMatcher, "_fp_one", lambda self, F, p, *a: singles.append((F.mnId - 40, p.mnId))
                        or one(self, F, p, *a))
    monkeypatch.setattr(matcher, "local_search_arrays",
                        lambda *a, **k: launches.append((len(a[0]), len(a[17]), int(a[18][-1]))) or arrays(*a, **k))
    return singles, launches


def predicted(golden, cfg, stats):
    jobs, _ = LC.build(golden, LC.CONFIGS[cfg][0])
    return [(s, jobs[s][1][i].mnId) for s, i in stats["redone"]]


@pytest.mark.parametrize("cfg", range(len(LC.CONFIGS)))
def test_device_path_equals_the_golden_and_the_loop(golden, monkeypatch, cfg):
    """search_local_points: the reference's return values, slots, visibility counts and every attribute's value and
    type from one launch per call; exactly the items the oracle predicts (marked, overtaken, stale) redone alone, and
    fewer than the cap; the loop on a rebuilt world gives the same."""
    from pyorbslam_amd import matcher
    singles, launches = count_calls(monkeypatch, matcher)
    monkeypatch.setattr(matcher.ORBMatcher, "_local_loop", lambda *a: pytest.fail("the loop"))
    stats = {}
    want = LC.drive(golden, LC.by_oracle(stats), cfg)
    got = LC.drive(golden, LC.by_matcher(matcher.ORBMatcher), cfg)
    assert LC.same(got, want), LC.diff(got, want)
    assert LC.same(got, LC.golden_results(golden, cfg))
    assert [x[:2] for x in launches] == [(1, 1)] * LC.N_FRAMES and sum(x[2] for x in launches) == stats["items"]
    assert singles == predicted(golden, cfg, stats) and 0 < len(singles) < REDO_CAP * stats["items"]
    monkeypatch.undo()
    loop = LC.drive(golden, LC.by_loop(LO.frustum_one, lambda F, vp, th, nn: matcher.ORBMatcher(
        nn, True).search_by_projection_f_p(F, vp, th)), cfg)
    assert LC.same(loop, got), LC.diff(loop, got)


@pytest.mark.parametrize("cfg", range(len(LC.CONFIGS)))
def test_many_equal_the_loop_and_the_golden_from_one_launch(golden, monkeypatch, cfg):
    from pyorbslam_amd import matcher
    loop = LC.drive(golden, LC.by_matcher(matcher.ORBMatcher), cfg)
    singles, launches = count_calls(monkeypatch, matcher)
    stats = {}
    LC.drive(golden, LC.by_oracle(stats), cfg)
    got = LC.drive(golden, LC.by_matcher(matcher.ORBMatcher, many=True), cfg)
    assert [x[:2] for x in launches] == [(LC.N_FRAMES, LC.N_FRAMES)] and singles == predicted(golden, cfg, stats)
    assert LC.same(got, loop) and LC.same(got, LC.golden_results(golden, cfg))


def test_genuine_marked_item_is_redone_alone(golden, monkeypatch):
    """A real ORBFE_FUSE_MARGINAL through the public call: a map point moved so that a feature lies exactly one radius
    from its projection.  That item takes the single-item logic, and the result is the loop's."""
    from fuse_cases import D, pt
    from pyorbslam_amd import _lib, matcher
    import matcher_world as MW
    n = 3
    a = dict(x=np.array([100, 293, 490], np.float32), y=np.array([100, 100, 100], np.float32),
             octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32), desc=np.stack([D(k) for k in range(n)]),
             uR=np.full(n, -1, np.float32), word=np.zeros(n, np.int32))
    runs = []
    for device in (True, False):
        w = MW.World()
        F = LC.Frame(w, a, np.eye(4))
        F.fx = F.fy = 64.0
        F.cx = F.cy = 0.0
        F.mbf = 32.0
        vp = []
        # level 0, scale factor 1, viewing cosine 1: the radius is 2.5 px and feature 1 lies exactly that far from
        # point 1's projection
        for i, (u, v) in enumerate(((100.5, 100.0), (290.5, 100.0), (490.25, 100.0))):
            row = pt(u, v)[0]
            row[8] = row[8] / 1.25 ** -0.5 * 1.2 ** -0.5   # the stand-in's log scale factor is log(1.2)
            p = LC.MapPoint(w, i, np.array(row[0:3]), D(), np.array(row[3:6]), row[6] / 0.8, row[8])
            p._pos, p._normal = np.array(row[0:3]).reshape(3, 1), np.array(row[3:6]).reshape(3, 1)
            w.mps.append(p)
            vp.append(p)
        if device:
            seen = []
            arrays = matcher.local_search_arrays
            monkeypatch.setattr(matcher, "local_search_arrays", lambda *a, **k: seen.append(arrays(*a, **k)) or seen[-1])
            singles, _ = count_calls(monkeypatch, matcher)
            res = matcher.ORBMatcher(1, False).search_local_points(F, vp, 1)
            assert len(seen) == 1 and seen[0]["status"].tolist() == [0, _lib.ORBFE_FUSE_MARGINAL, 0]
            assert [s[1] for s in singles] == [1]
            monkeypatch.undo()
        else:
            res = LO.loop(F, vp, 1, 0.5, 1)
        runs.append((res, MW.encode_mps(w, F.mvpMapPoints).tolist()))
    assert runs[0] == runs[1] == ((3, 2), [0, -1, 2])


# ---- 4. the C3 tracking loop's first frames --------------------------------------------------------------------------
def test_c3_frames_through_the_gpu_extractor(monkeypatch):
    """Frames 1-3 of the C3 golden through the GPU extractor and search_local_points: the in-view set, the levels and
    projections, fp_n and fp_assign equal the golden's, from one launch per frame with exactly the oracle's redos."""
    import seq_harness as H
    from pyorbslam_amd import frame as F
    from pyorbslam_amd import matcher
    from pyorbslam_amd.pyORBExtractor import ORBextractor
    from test_local_search_cpu import c3_scenes, check_c3

    class DropInFrame(H.SeqFrame):
        pass

    F.install(DropInFrame)
    launches, ones = [], []
    arrays, inner = matcher.local_search_arrays, matcher.ORBMatcher._fp_one
    monkeypatch.setattr(matcher, "local_search_arrays", lambda *a, **k: launches.append(1) or arrays(*a, **k))
    monkeypatch.setattr(matcher.ORBMatcher, "_fp_one", lambda self, Fr, p, th: ones.append(p) or inner(self, Fr, p, th))
    monkeypatch.setattr(matcher.ORBMatcher, "_local_loop", lambda *a: pytest.fail("the loop"))
    g, kinds, scenes = c3_scenes((ORBextractor(**H.PARAMS), ORBextractor(**H.PARAMS)), DropInFrame)
    check_c3(monkeypatch, matcher, scenes, g, kinds, launches, ones)
