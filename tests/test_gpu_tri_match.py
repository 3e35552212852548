"""k_tri_match on the GPU: the host entry on every crafted case against the array oracle, bit for bit on all
outputs and with guard rows around them, the reference's golden, search_for_triangulation_many against loops of the
single search, its per-element fallbacks, and concurrent callers."""
import ctypes as C
import threading

import numpy as np
import pytest

import tri_match_cases as TC
import tri_match_oracle as O
from test_tri_match_cpu import golden_world

pytestmark = pytest.mark.gpu

CASES = TC.all_cases()
ORACLE = {c["name"]: TC.oracle(c) for c in CASES}  # computed once, shared, never modified
GUARD = -9
ARRAYS = ("desc", "angle", "xy", "octave", "flags", "off", "fv_off", "fv_node", "fv_end", "fv_idx", "lvl_off",
          "thr_epi", "thr_ex")


def run_host(case):
    from pyorbslam_amd.matcher import tri_match_arrays
    a = TC.pack(case["frames"])
    return tri_match_arrays(*[a[k] for k in ARRAYS], np.array(case["pairs"], np.int32).reshape(-1, 2),
                            np.stack(case["F12"]) if case["pairs"] else np.zeros((0, 9)),
                            np.array(case["epi"], np.float64).reshape(-1, 2), case["th"], case["only_stereo"])


def assert_raw(case, got, want, where=""):
    for p, ((a, _), w) in enumerate(zip(case["pairs"], want)):
        n1 = len(case["frames"][a]["desc"])
        tag = f"{case['name']}{where} pair {p}"
        assert np.array_equal(got["match12"][p, :n1], w[0]), tag
        assert np.array_equal(got["bin12"][p, :n1], w[1]), tag
        assert np.array_equal(got["hist"][p], w[2]), tag
        assert int(got["n_raw"][p]) == w[3] and int(got["status"][p]) == w[4] and int(got["stopped"][p]) == w[5], tag
        assert bool((got["match12"][p, n1:] == -1).all()) and bool((got["bin12"][p, n1:] == -1).all()), tag


def run_guarded(case):
    """The ABI entry itself with guard rows before and behind every output and guard entries behind every row."""
    from pyorbslam_amd import _lib
    a = TC.pack(case["frames"])
    P = len(case["pairs"])
    stride = max(len(f["desc"]) for f in case["frames"]) + 3
    o = dict(match12=np.full((P + 2, stride), GUARD, np.int32), bin12=np.full((P + 2, stride), GUARD, np.int8),
             hist=np.full((P + 2, 32), GUARD, np.int32), n_raw=np.full(P + 2, GUARD, np.int32),
             status=np.full(P + 2, GUARD, np.int32), stopped=np.full(P + 2, GUARD, np.int32))
    out = _lib.TriMatchOut(**{k: v[1:].ctypes.data for k, v in o.items()})
    pairs = np.array(case["pairs"], np.int32).reshape(-1, 2)
    F12, epi = np.ascontiguousarray(np.stack(case["F12"])), np.array(case["epi"], np.float64)
    _lib.call("orbfe_tri_match", *[_lib.ptr(a[k]) for k in ARRAYS[:6]], len(case["frames"]),
              *[_lib.ptr(a[k]) for k in ARRAYS[6:]], _lib.ptr(pairs), _lib.ptr(F12), _lib.ptr(epi), P, case["th"],
              int(case["only_stereo"]), C.byref(out), stride)
    return o


# ---- 1. host entry: every case, all six raw outputs, bit for bit ------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_entry_matches_the_oracle(case):
    from pyorbslam_amd import _lib
    want = ORACLE[case["name"]]
    case["check"](want)
    assert (sum(w[3] for w in want) == 0) == case["empty"]
    got = run_host(case)
    assert_raw(case, got, want)
    if case["name"] == "marginal":
        assert got["status"].tolist() == [0, _lib.ORBFE_TRI_MARGINAL, 0]
    else:
        assert not got["status"].any()


@pytest.mark.parametrize("name", ["sharing_nine_pairs", "run2_129", "walk_stops", "empty_frames"])
def test_guard_rows_stay_intact(name):
    case = next(c for c in CASES if c["name"] == name)
    o = run_guarded(case)
    P = len(case["pairs"])
    for k, v in o.items():
        assert bool((v[0] == GUARD).all()) and bool((v[P + 1] == GUARD).all()), k
    for p, ((a, _), w) in enumerate(zip(case["pairs"], ORACLE[name])):
        n1 = len(case["frames"][a]["desc"])
        assert np.array_equal(o["match12"][1 + p, :n1], w[0]) and np.array_equal(o["bin12"][1 + p, :n1], w[1])
        assert bool((o["match12"][1 + p, n1:] == GUARD).all()) and bool((o["bin12"][1 + p, n1:] == GUARD).all())
        assert np.array_equal(o["hist"][1 + p], w[2])
        assert (int(o["n_raw"][1 + p]), int(o["status"][1 + p]), int(o["stopped"][1 + p])) == (w[3], w[4], w[5])


def test_no_pairs_launch_nothing():
    from pyorbslam_amd import _lib
    got = run_host(dict(CASES[0], pairs=[], F12=[], epi=[]))
    assert got["match12"].shape[0] == 0 and got["status"].shape == (0,) and got["stopped"].shape == (0,)
    ms = C.c_float(-1)
    assert _lib.lib().orbfe_tri_match_last_ms(C.byref(ms)) == 0 and ms.value >= 0


# ---- 2. the reference's golden ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return golden_world()


def test_golden_through_the_host_entry(golden):
    from pyorbslam_amd.matcher import ORBMatcher, tri_match_arrays
    z, runs = golden
    frames = [TC.world_frame(z, j) for j in range(int(z["n_kf"]))]
    a = TC.pack(frames)
    pairs = np.array([[0, j] for j, _, _ in runs], np.int32)
    F12 = np.stack([F for _, F, _ in runs])
    epi = np.array([TC.world_epipole(z["kf0_T"], z[f"kf{j}_T"]) for j, _, _ in runs])
    for only in (False, True):
        got = tri_match_arrays(*[a[k] for k in ARRAYS], pairs, F12, epi, 50, only)
        assert not got["status"].any() and not got["stopped"].any()
        for p, (_, _, lst) in enumerate(runs):
            for o, ori, _, want in lst:
                if o == only:
                    r = ORBMatcher(0.6, ori)._tri_reject(got["match12"][p, :300], got["bin12"][p, :300], got["hist"][p])
                    assert r == [tuple(x) for x in want.tolist()], (only, p, ori)


# ---- 3. the _many drop-in ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cand", [1, 3, 8])
@pytest.mark.parametrize("only", [False, True])
@pytest.mark.parametrize("ori", [True, False])
def test_many_equal_a_loop_of_single_searches(golden, n_cand, only, ori):
    from pyorbslam_amd.matcher import ORBMatcher
    z, runs = golden
    w = TC.build_world(z)
    m = ORBMatcher(0.6, ori)
    kfs, F = w.kfs[1:1 + n_cand], [r[1] for r in runs[:n_cand]]
    want = [m.search_for_triangulation(w.kfs[0], kf, f, only) for kf, f in zip(kfs, F)]
    got = m.search_for_triangulation_many(w.kfs[0], kfs, F, only)
    assert got == want and sum(len(x) for x in got) > 0
    assert all(type(i) is int and type(k) is int for x in got for i, k in x)
    for x, (_, _, lst) in zip(got, runs):
        assert x == [tuple(p) for p in next(e[3] for e in lst if e[0] == only and e[1] == ori).tolist()]


def test_many_fall_back_per_element(golden, monkeypatch):
    """A float32 F12 in one element and a pair that comes back MARGINAL: those two take the single search, the others
    the one launch; a stop case in position j raises StopIteration."""
    from pyorbslam_amd import _lib, matcher
    z, runs = golden
    w = TC.build_world(z)
    m = matcher.ORBMatcher(0.6, True)
    kfs, F = w.kfs[1:6], [r[1] for r in runs[:5]]
    F[1] = F[1].astype(np.float32)
    want = [m.search_for_triangulation(w.kfs[0], kf, f) for kf, f in zip(kfs, F)]
    singles, launches = [], []
    single, arrays = m.search_for_triangulation, matcher.tri_match_arrays

    def launch(*a, **k):
        launches.append(len(a[13]))
        r = arrays(*a, **k)
        r["status"][2] = _lib.ORBFE_TRI_MARGINAL  # the third live pair: element 3
        return r
    monkeypatch.setattr(m, "search_for_triangulation", lambda a, b, f, o=False: singles.append(b) or single(a, b, f, o))
    monkeypatch.setattr(matcher, "tri_match_arrays", launch)
    assert m.search_for_triangulation_many(w.kfs[0], kfs, F) == want
    assert singles == [kfs[1], kfs[3]] and launches == [4]
    # the walk of element 2 stops: the loop raises there, and so does the many call
    kfs[2].mFeatVec = {-1: [0]}
    with pytest.raises(StopIteration):
        [single(w.kfs[0], kf, f) for kf, f in zip(kfs, F)]
    del singles[:], launches[:]
    with pytest.raises(StopIteration):
        m.search_for_triangulation_many(w.kfs[0], kfs, F)
    assert singles == [kfs[1]] and launches == [4]


def test_marginal_pair_is_redone_by_the_single_search(monkeypatch):
    """A real MARGINAL through the drop-in: a neighbour whose level thresholds are exactly 4.0, the squared distance
    of a candidate two rows off the line.  That element takes the single search, the other stays in the launch."""
    import matcher_world as MW
    from pyorbslam_amd import _lib, matcher
    n = 6
    a = dict(x=np.full(n, 100, np.float32), y=np.array([50, 52, 80, 80, 90, 90], np.float32),
             octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32), desc=np.stack([TC.D(k) for k in range(n)]),
             uR=np.full(n, -1, np.float32), word=np.zeros(n, np.int32))
    w = MW.World()
    T2 = np.eye(4, dtype=np.float32)
    T2[0, 3] = T2[2, 3] = 1.0
    k1, k2, k3 = MW.KeyFrame(w, 0, a, np.eye(4, dtype=np.float32)), MW.KeyFrame(w, 1, a, T2), MW.KeyFrame(w, 2, a, T2)
    s = 4.0 / 3.84
    s = next(c for c in (s, float(np.nextafter(s, 0.0)), float(np.nextafter(s, 2.0))) if 3.84 * c == 4.0)
    k2.mvLevelSigma2 = [s] * 8
    m = matcher.ORBMatcher(0.6, False)
    seen, singles = [], []
    arrays, single = matcher.tri_match_arrays, m.search_for_triangulation
    want = [single(k1, k, TC.F_ROW) for k in (k2, k3)]
    monkeypatch.setattr(matcher, "tri_match_arrays", lambda *a, **k: seen.append(arrays(*a, **k)) or seen[-1])
    monkeypatch.setattr(m, "search_for_triangulation", lambda a, b, f, o=False: singles.append(b) or single(a, b, f, o))
    assert m.search_for_triangulation_many(k1, [k2, k3], [TC.F_ROW, TC.F_ROW]) == want and len(want[1]) > 0
    assert len(seen) == 1 and seen[0]["status"].tolist() == [_lib.ORBFE_TRI_MARGINAL, 0] and singles == [k2]


# ---- 4. four threads ----------------------------------------------------------------------------------------------
def test_four_threads_get_their_own_results():
    names = ["run2_129", "epipole_gate_only_when_both_mono", "sharing_nine_pairs", "more_nodes_than_waves"]
    cases = [next(c for c in CASES if c["name"] == k) for k in names]
    errors = []

    def work(case):
        try:
            for _ in range(5):
                assert_raw(case, run_host(case), ORACLE[case["name"]], " (threads)")
        except BaseException as e:  # noqa: BLE001
            errors.append((case["name"], repr(e)))
    ts = [threading.Thread(target=work, args=(c,)) for c in cases]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
