"""k_ff_search without a GPU: every placed case's claim on the array oracle, the margin cases, the reference's golden
and the six matcher_ff fixtures through the oracle and the replay, the redo cap, search_by_projection_f_f_many with the
oracle in the kernel's place (the replay's situations and the fallbacks), and the entry's validation, which runs before
any device call."""
import numpy as np
import pytest

import ff_cases as FC
import ff_margin_cases as FM
import ff_oracle as FO
import matcher_frames as MF
from bow_match_cases import D
from conftest import GOLDEN
from pyorbslam_amd import _lib as LIB

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")

CASES = FC.all_cases()
SETS = FM.all_sets()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "ff_many.npz", allow_pickle=False)


# ---- the cases -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_holds_its_claim(case):
    out = FC.oracle(case)
    case["check"](out)
    assert np.flatnonzero(out["status"]).tolist() == case["marked"]
    assert [o.dtype for o in out.values()] == [np.int32, np.int32, np.uint8]


@pytest.mark.parametrize("S", SETS, ids=[S.name for S in SETS])
def test_margins_are_sound_at_the_flip(S):
    """On every rung an unmarked item decides as the reference body does; the reference's decision flips between the
    two innermost rungs, one unit in the last place apart, and both are marked; the mark ends inside the ladder."""
    a = FM.arrays(S)
    assert a["eps"] == (FO.EPS_F32 if S.dtype is np.float32 else FO.EPS_F64)
    bi, bd, st = FO.search(a)
    ref = FM.reference(S)
    assert S.found[0] and not S.found[1] and S.found == [True, False] * (FM.J + 1)
    assert abs(FM._ordinal(S.values[0], S.dtype) - FM._ordinal(S.values[1], S.dtype)) == 1
    for i in range(len(S.values)):
        if st[i]:
            continue
        if S.gate == "depth":
            assert FM.oracle_depth_negative(a, i) == (not S.found[i]), (S.name, i)
            assert ref[i] == (-1, -1) == (int(bi[i]), int(bd[i]))
        else:
            assert (int(bi[i]), int(bd[i])) == ref[i] and (ref[i][0] >= 0) == S.found[i], (S.name, i)
    assert st[0] and st[1]
    # float64's eps is 16 units in the last place and ur's bound adds bf's term: that ladder alone stays open
    assert (not st[-1] and not st[-2]) or S.name == "stereo_f64"


# ---- the goldens through the oracle and the replay -----------------------------------------------------------------------

def test_oracle_and_replay_give_the_golden_under_the_cap(golden):
    """ff_many.npz: the reference's counts and slots; the items the oracle predicts to be redone (marked, overtaken, not
    expressible) are more than none and fewer than 5 % of those sent; features are assigned twice; and the stereo
    gate decides (without it the result is another)."""
    jobs, objs = FC.load_world(golden)
    stats = {}
    got = FO.replay(jobs, stats=stats)
    assert FC.same((got, FC.state(jobs, objs)), FC.golden_results(golden))
    assert [FO.mode_of(c, x) for c, x, _ in jobs] == [0, 1, 2, 0, 1, 2]
    assert [c.mTcw.dtype for c, _, _ in jobs] == [np.float32] * 3 + [np.float64] * 3
    assert 0 < len(stats["redone"]) < FC.REDO_CAP * stats["items"], stats
    assert len(stats["redone"]) == stats["marginal"] + stats["taken"] + stats["alone"]
    assert stats["taken"] > 0 and stats["twice"] > 0
    jobs, objs = FC.load_world(golden)
    other = FO.replay(jobs, results=lambda a: FO.search(a, stereo_gate=False))
    assert not FC.same((other, FC.state(jobs, objs)), FC.golden_results(golden))


def test_the_loop_of_the_reference_body_gives_the_golden(golden):
    jobs, objs = FC.load_world(golden)
    got = [FO.loop(c, x, th) for c, x, th in jobs]
    assert FC.same((got, FC.state(jobs, objs)), FC.golden_results(golden))


def test_oracle_and_replay_give_the_six_fixtures():
    """matcher_ff_*.npz, for equality only: their points collide by construction."""
    jobs, objs, want = FC.load_fixtures()
    got = FO.replay(jobs)
    assert got == [w[0] for w in want]
    for s, w in zip(FC.state(jobs, objs), want):
        assert np.array_equal(s, w[1])


# ---- the public call with the oracle in the kernel's place -----------------------------------------------------------------

def fake_device(monkeypatch, matcher, launches):
    def arrays(*args):
        a = dict(zip(FO.ARRAYS + ("eps",), args))
        launches.append((len(a["kf_f64"]), len(a["srch_kf"]), int(a["srch_off"][-1])))
        return dict(zip(FO.OUTPUTS, FO.search(a)))
    monkeypatch.setattr(LIB, "device_present", lambda: True)
    monkeypatch.setattr(matcher, "ff_search_arrays", arrays)


def counting(monkeypatch, matcher, singles):
    """The single call answered by the reference body's loop, and recorded; _ff_one recorded."""
    ones, inner = [], matcher.ORBMatcher._ff_one
    monkeypatch.setattr(matcher.ORBMatcher, "_ff_one",
                        lambda self, cur, last, i, *a: ones.append((id(cur), i)) or inner(self, cur, last, i, *a))
    monkeypatch.setattr(matcher.ORBMatcher, "search_by_projection_f_f",
                        lambda self, c, x, th: singles.append((id(c), th)) or FO.loop(c, x, th, self.mbCheckOrientation))
    return ones


def test_many_replays_the_golden_from_one_launch(golden, monkeypatch):
    from pyorbslam_amd import matcher
    launches, singles = [], []
    fake_device(monkeypatch, matcher, launches)
    ones = counting(monkeypatch, matcher, singles)
    jobs, objs = FC.load_world(golden)
    stats = {}
    FO.replay(jobs, stats=stats)
    jobs, objs = FC.load_world(golden)
    got = matcher.ORBMatcher(0.8, True).search_by_projection_f_f_many(
        [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    assert FC.same((got, FC.state(jobs, objs)), FC.golden_results(golden))
    assert launches == [(FC.N_PAIRS, FC.N_PAIRS, stats["items"])] and singles == []
    assert ones == [(id(jobs[s][0]), i) for s, i in stats["redone"]]


def test_many_replays_the_six_fixtures_from_one_launch(monkeypatch):
    from pyorbslam_amd import matcher
    launches, singles = [], []
    fake_device(monkeypatch, matcher, launches)
    counting(monkeypatch, matcher, singles)
    jobs, objs, want = FC.load_fixtures()
    got = matcher.ORBMatcher(0.8, True).search_by_projection_f_f_many(
        [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    assert got == [w[0] for w in want] and [x[:2] for x in launches] == [(6, 6)] and singles == []
    for s, w in zip(FC.state(jobs, objs), want):
        assert np.array_equal(s, w[1])


# ---- the replay's situations, on small worlds ------------------------------------------------------------------------------

def world(feats, points, dtype=np.float64):
    """A pair: the current frame has the features (x, y, octave, angle, uR); the last frame one keypoint per point
    (feature aimed at, du, dv, descriptor, observations, angle, octave); a point lands (du, dv) px from its feature."""
    T = FM._pose(dtype)
    a = dict(x=np.array([f[0] for f in feats], np.float32), y=np.array([f[1] for f in feats], np.float32),
             octave=np.array([f[2] for f in feats], np.int32), angle=np.array([f[3] for f in feats], np.float32),
             desc=np.stack([D(9)] * len(feats)), uR=np.array([f[4] for f in feats], np.float32))
    cur = FC.Frame(a, T)
    n = len(points)
    b = dict(x=np.zeros(n, np.float32), y=np.zeros(n, np.float32), octave=np.array([p[6] for p in points], np.int32),
             angle=np.array([p[5] for p in points], np.float32), desc=np.zeros((n, 32), np.uint8),
             uR=np.full(n, -1.0, np.float32))
    last = FC.Frame(b, T.copy())
    last.mvpMapPoints = [MF.MP(p[3], pos=FM._world(T, feats[p[0]][0] + p[1], feats[p[0]][1] + p[2], 9.0).astype(
        dtype).reshape(3, 1), obs=p[4]) for p in points]
    return cur, last


SPOTS = [((c + 0.2) / FM.WINV, (20 + 0.2) / FM.HINV) for c in (10, 20, 30, 40)]


def overwrite_world():
    """Feature 0 is taken by a point without observations and then by another: counted twice, in a rotation bin (two
    entries) that loses against the three bins of features 1-3 (three entries each), so it is rejected twice."""
    feats = [(x, y, 0, 0.0, -1.0) for x, y in SPOTS]
    points = [(0, 0.5, 0.25, D(9, 1), 0, 100.0, 0), (0, -0.5, 0.25, D(9, 2), 0, 100.0, 0)]
    for f, ang in ((1, 10.0), (2, 40.0), (3, 70.0)):
        points += [(f, 0.25 * k, 0.5, D(9, k), 0, ang, 0) for k in range(3)]
    return world(feats, points)


def overtaken_world():
    """Two features side by side, two points that both prefer feature 0: the first, with observations, takes it; the
    second is redone alone and gets feature 1."""
    x, y = SPOTS[0]
    cur, last = world([(x, y, 0, 0.0, -1.0), (x + 2.0, y, 0, 0.0, -1.0)],
                      [(0, 0.5, 0.25, D(9), 2, 0.0, 0), (0, 0.75, 0.25, D(9), 2, 0.0, 0)])
    cur.mDescriptors = np.stack([D(9), D(9, 1, 2)])
    return cur, last


def run_many(monkeypatch, pairs, ths, check_ori=True):
    from pyorbslam_amd import matcher
    launches, singles = [], []
    fake_device(monkeypatch, matcher, launches)
    ones = counting(monkeypatch, matcher, singles)
    got = matcher.ORBMatcher(0.8, check_ori).search_by_projection_f_f_many([p[0] for p in pairs], [p[1] for p in pairs],
                                                                            ths)
    return got, launches, singles, ones


def slots(cur, last):
    return [-1 if m is None else last.mvpMapPoints.index(m) for m in cur.mvpMapPoints]


@pytest.mark.parametrize("check_ori", [True, False])
def test_a_feature_assigned_twice_is_counted_and_rejected_twice(monkeypatch, check_ori):
    cur, last = overwrite_world()
    stats = {}
    want = FO.loop(cur, last, 7.0, check_ori, stats)
    left = slots(cur, last)
    assert stats["twice"] == 7 and want == (9 if check_ori else 11) and left[0] == (-1 if check_ori else 1)
    cur, last = overwrite_world()
    got, launches, singles, ones = run_many(monkeypatch, [(cur, last)], 7.0, check_ori)
    assert got == [want] and slots(cur, last) == left and launches == [(1, 1, 11)] and ones == [] and singles == []


def test_an_overtaken_item_is_redone_and_gets_its_next_best(monkeypatch):
    cur, last = overtaken_world()
    want = FO.loop(cur, last, 7.0, False)
    assert want == 2 and slots(cur, last) == [0, 1]
    cur, last = overtaken_world()
    got, launches, _, ones = run_many(monkeypatch, [(cur, last)], 7.0, False)
    assert got == [2] and slots(cur, last) == [0, 1] and launches == [(1, 1, 2)] and ones == [(id(cur), 1)]


def test_a_point_with_a_flat_position_is_redone_alone(monkeypatch):
    """get_world_pos() of shape (3,): the reference's expressions broadcast it; the arrays do not take it."""
    def make():
        cur, last = overtaken_world()
        p = last.mvpMapPoints[0]
        p._p = p._p.reshape(3)
        return cur, last
    cur, last = make()
    want = FO.loop(cur, last, 7.0, False)
    left = slots(cur, last)
    cur, last = make()
    got, launches, _, ones = run_many(monkeypatch, [(cur, last)], 7.0, False)
    assert got == [want] and slots(cur, last) == left and launches == [(1, 1, 1)]
    assert ones[0] == (id(cur), 0)


def test_duplicates_run_the_loop(monkeypatch):
    """A current frame twice, a slot list twice, or a current frame that is also a last frame: the plain loop, no
    launch."""
    for kind in ("frame", "slots", "also_last"):
        a, b = overtaken_world(), overtaken_world()
        if kind == "frame":
            pairs = [a, (a[0], b[1])]
        elif kind == "slots":
            b[0].mvpMapPoints = a[0].mvpMapPoints
            pairs = [a, b]
        else:
            pairs = [a, (b[0], a[0])]
            a[0].mvbOutlier = [False] * a[0].N
        got, launches, singles, _ = run_many(monkeypatch, pairs, 7.0, False)
        assert launches == [] and [s[0] for s in singles] == [id(p[0]) for p in pairs], kind
        monkeypatch.undo()


def test_a_shared_last_frame_uses_one_launch(monkeypatch):
    a, b = overtaken_world(), overtaken_world()
    got, launches, singles, _ = run_many(monkeypatch, [a, (b[0], a[1])], [7.0, 14.0], False)
    assert got == [2, 2] and launches == [(2, 2, 4)] and singles == []
    assert slots(*a) == [0, 1] and slots(b[0], a[1]) == [0, 1]


def test_a_pair_that_cannot_be_packed_takes_the_single_call(monkeypatch):
    """An np.float32 th, a pose that is not finite, an int pose, a missing mbf, an octave outside the scale table, a
    slot list of the wrong length: that pair takes the single call at its place, the others share the launch."""
    def spoil(kind, cur, last):
        if kind == "pose_nan":
            last.mTcw = last.mTcw.copy()
            last.mTcw[0, 3] = np.nan
        elif kind == "pose_int":
            cur.mTcw = np.eye(4, dtype=np.int64)
        elif kind == "no_mbf":
            cur.mbf = np.float32(cur.mbf)
        elif kind == "octave":
            last.mvKeys[0].octave = FC.LEVELS
        elif kind == "slots":
            cur.mvpMapPoints = cur.mvpMapPoints + [None]
    for kind in ("th_f32", "th_inf", "pose_nan", "pose_int", "no_mbf", "octave", "slots"):
        worlds = [overtaken_world() for _ in range(3)]
        ths = [7.0, np.float32(7.0) if kind == "th_f32" else float("inf") if kind == "th_inf" else 7.0, 7]
        spoil(kind, *worlds[1])
        from pyorbslam_amd import matcher
        launches, singles = [], []
        fake_device(monkeypatch, matcher, launches)
        monkeypatch.setattr(matcher.ORBMatcher, "search_by_projection_f_f",
                            lambda self, c, x, th: singles.append(id(c)) or -7)
        got = matcher.ORBMatcher(0.8, False).search_by_projection_f_f_many([w[0] for w in worlds],
                                                                          [w[1] for w in worlds], ths)
        assert got == [2, -7, 2] and launches == [(2, 2, 4)] and singles == [id(worlds[1][0])], kind
        monkeypatch.undo()


def test_without_a_device_the_loop_runs(monkeypatch):
    from pyorbslam_amd import matcher
    worlds = [overtaken_world() for _ in range(2)]
    monkeypatch.setattr(LIB, "device_present", lambda: False)
    monkeypatch.setattr(matcher, "ff_search_arrays", lambda *a: pytest.fail("a launch"))
    monkeypatch.setattr(matcher.ORBMatcher, "search_by_projection_f_f", lambda self, c, x, th: th)
    m = matcher.ORBMatcher(0.8, True)
    assert m.search_by_projection_f_f_many([w[0] for w in worlds], [w[1] for w in worlds], (7.0, 14.0)) == [7.0, 14.0]
    with pytest.raises(ValueError):
        m.search_by_projection_f_f_many([w[0] for w in worlds], [w[1] for w in worlds], [7.0])
    with pytest.raises(ValueError):
        m.search_by_projection_f_f_many([worlds[0][0]], [], 7.0)


# ---- the entry's validation, before any device call ------------------------------------------------------------------------

def host(a):
    from pyorbslam_amd.matcher import ff_search_arrays
    return ff_search_arrays(*[a[k] for k in FO.ARRAYS], a["eps"])


def test_zero_searches_and_zero_items_succeed_without_a_launch():
    for name in ("zero_searches", "zero_items"):
        out = host(FC.arrays(FC.by_name(name)))
        assert list(out) == list(FO.OUTPUTS) and all(len(v) == 0 for v in out.values())


@pytest.mark.parametrize("what", ["th_nan", "th_inf", "mode_low", "mode_high", "level_low", "level_high", "pos_nan",
                                  "bf_nan", "uright_nan", "item_pt", "eps"])
def test_bad_arguments_are_refused_before_any_device_call(what):
    a = FC.arrays(FC.by_name("two_searches_one_frame_two_ths_two_modes"))
    assert np.isnan(a["pt_f64"][:, 3:]).all()      # the slots that are not read hold NaN and are not refused for it
    if what.startswith("th_"):
        a["srch_th"][1] = np.nan if what == "th_nan" else np.inf
    elif what.startswith("mode_"):
        a["srch_mode"][0] = -1 if what == "mode_low" else 3
    elif what.startswith("level_"):
        a["item_level"][1] = -1 if what == "level_low" else 4
    elif what == "pos_nan":
        a["pt_f64"][0, 2] = np.nan
    elif what == "bf_nan":
        a["kf_f64"][0, 4] = np.nan
    elif what == "uright_nan":
        a["u_right"][0] = np.nan
    elif what == "item_pt":
        a["item_pt"][0] = 1
    else:
        a["eps"] = float("nan")
    with pytest.raises(LIB.OrbfeError) as e:
        host(a)
    assert e.value.code == LIB.ORBFE_EINVAL


def test_the_header_declares_the_entry_and_the_abi_stays():
    from conftest import ROOT
    text = (ROOT / "include" / "orbfe.h").read_text()
    assert "int orbfe_ff_search(" in text and "int orbfe_ff_search_last_ms(float* ms);" in text
    assert "#define ORBFE_ABI_VERSION 9" in text and LIB.lib().orbfe_abi_version() == 9
    assert LIB.has("orbfe_ff_search") and LIB.has("orbfe_ff_search_last_ms")
