"""k_local_search without a GPU: every placed case's claim on the array oracle, the reference's golden through the
oracle and the replay, the public calls with the oracle in the kernel's place, is_in_frustum_many against the golden's
attribute values and types, the fallbacks, and the entry's ABI and validation (which runs before any device call)."""
import ctypes as C
import re

import numpy as np
import pytest

import local_search_cases as LC
import local_search_oracle as LO
from conftest import GOLDEN, ROOT
from pyorbslam_amd import _lib as LIB

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")

CASES = LC.all_cases()
NEW = ("orbfe_local_search", "orbfe_local_search_last_ms")
REDO_CAP = 0.05


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "local_search.npz", allow_pickle=False)


# ---- the cases -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_holds_its_claim(case):
    out = LC.oracle(case)
    case["check"](out)
    assert np.flatnonzero(out["status"]).tolist() == case["marked"]
    assert [o.dtype for o in out.values()] == [np.uint8] + [np.int32] * 5 + [np.uint8]


def test_two_minima_are_the_sequential_update():
    """The two smallest keys (distance, visiting position) are what the reference's update holds after the last
    candidate, on every case and on random candidate lists with many ties."""
    rng = np.random.Generator(np.random.PCG64(3))
    lists = [[(int(d), pos, 100 + pos) for pos, d in enumerate(rng.integers(0, 4, int(rng.integers(0, 9))))]
             for _ in range(300)]
    for case in CASES:
        a = LC.arrays(case)
        lists += [LO.candidates(a, LO.search_of(a, i), i)[3] for i in range(int(a["srch_off"][-1]) if len(
            a["srch_off"]) else 0)]
    assert sum(len(c) >= 3 for c in lists) > 100
    for cand in lists:
        two = sorted(cand)[:2] + [(-1, -1, -1)] * 2
        assert LO.sequential(cand) == (two[0][2], two[0][0], two[1][2], two[1][0])


def test_the_set_is_not_vacuous():
    names = {c["name"] for c in CASES}
    sizes = [len(it) for it in LC.by_name("ragged_0_1_255_256_257")["items"]]
    assert {0, 1, 255, 256, 257} <= set(sizes) and LC.CHUNK == 256
    assert {"window_15", "window_16", "window_17", "best_and_second_in_one_lane", "best_and_second_in_two_lanes",
            "tie_in_one_lane", "single_candidate_has_no_second", "blocked_best", "blocked_second",
            "blocked_third_changes_nothing", "th_1_flag_off", "th_1_0000001_flag_on", "zero_searches",
            "zero_items"} <= names
    marked = sum(len(c["marked"]) for c in CASES)
    items = sum(len(it) for c in CASES for it in c["items"])
    assert 10 <= marked < 0.05 * items


# ---- the golden -----------------------------------------------------------------------------------------------------------

def test_oracle_and_replay_reproduce_the_reference(golden):
    """Every configuration: the oracle with its redo gives the reference's results, slots, visibility counts and
    every attribute's value, dtype and shape; the redone items stay under the cap; the events the file was chosen
    for are there."""
    stats = {}
    for cfg in range(len(LC.CONFIGS)):
        got = LC.drive(golden, LC.by_oracle(stats), cfg)
        want = LC.golden_results(golden, cfg)
        assert LC.same(got, want), (cfg, LC.diff(got, want))
        assert int(want[0][:, 1].max()) >= 20
    assert stats["taken"] > 0 and stats["stale"] > 0 and stats["ratio"] > 0
    assert 0 < len(stats["redone"]) < REDO_CAP * stats["items"]
    kinds = {int(k) for cfg in range(len(LC.CONFIGS)) for k in np.unique(golden[f"ls_kind{cfg}"])}
    assert kinds == {-1, 41, 42, 81, 82}   # float32 and float64, shape (1,) and shape (1, 1)
    assert golden["mp_bad"].any() and (golden["ls_obs"] > 0).any() and (golden["ls_obs"] == 0).any()


def test_the_loop_on_the_stand_ins_reproduces_the_reference(golden):
    """The reference's two bodies as restated in the oracle module (what an item is redone with)."""
    for cfg in range(len(LC.CONFIGS)):
        got = LC.drive(golden, LC.by_loop(LO.frustum_one, lambda F, vp, th, nn: sum(
            LO.fp_one(F, p, th, nn) for p in vp if p.mbTrackInView and not p.is_bad())), cfg)
        assert LC.same(got, LC.golden_results(golden, cfg)), cfg


@pytest.mark.parametrize("seed", [61, 62, 63])
def test_unmarked_items_decide_as_the_reference_and_few_are_marked(seed):
    """The soundness of the bound on random worlds with float32 and float64 poses, at the golden's two values of th:
    wherever the oracle leaves the status 0, in_view, the level, the winner, both distances and the second's octave
    are those of the reference's two bodies on the objects.  At most 2 % of the items that reach a cell window may be
    marked."""
    import fuse_cases as FC
    import margin_cases as M
    g = FC.Z(LC.make_extras(FC.clone_world(seed), seed))
    items = reached = marked = found = 0
    for dtype, th in ((np.float32, 1), (np.float64, 5), (np.float32, 5), (np.float64, 1)):
        jobs, _ = LC.build(g, dtype)
        a, where = LO.pack(jobs, th, LC.LIMIT)
        assert a["eps"] == (LO.EPS_F32 if dtype == np.float32 else LO.EPS_F64)
        out = LO.search(a)
        for s, (F, vp) in enumerate(jobs):
            base = int(a["off"][s])
            for c, i in enumerate(where[s]):
                j = int(a["srch_off"][s]) + c
                got = tuple(int(o[j]) for o in out)
                items += 1
                if LO._window(a, s, j)[2][2] is not None:
                    reached += 1
                    marked += int(got[-1] != 0)
                if got[-1]:
                    continue
                ref, _ = M.local_reference(F, vp[i], LC.LIMIT, th)
                assert M.same_as_reference("local", got, ref, lambda f: int(a["octave"][base + f])), (s, i, got, ref)
                found += ref[2] >= 0
    print(f"items {items} reached {reached} marked {marked} share {marked / reached:.4f} found {found}")
    assert reached > 1000 and found > 500
    assert marked <= 0.02 * reached


# ---- the product with the oracle in the kernel's place -----------------------------------------------------------------

def fake_device(monkeypatch, matcher, launches):
    def arrays(*args):
        a = dict(zip(LO.ARRAYS + ("th", "th_on", "eps"), args))
        launches.append((len(a["kf_f64"]), len(a["srch_kf"]), int(a["srch_off"][-1])))
        return dict(zip(LO.OUTPUTS, LO.search(a)))
    monkeypatch.setattr(LIB, "device_present", lambda: True)
    monkeypatch.setattr(matcher, "local_search_arrays", arrays)


def counting(monkeypatch, cls, name):
    calls, inner = [], getattr(cls, name)

    def wrapped(self, *a, **k):
        calls.append(a)
        return inner(self, *a, **k)
    monkeypatch.setattr(cls, name, wrapped)
    return calls


@pytest.mark.parametrize("cfg", range(len(LC.CONFIGS)))
def test_device_path_replays_the_reference(golden, monkeypatch, cfg):
    """search_local_points and _many over the oracle's arrays: the golden's results and everything left behind, one
    launch per call (one for both frames of _many), exactly the items the oracle's replay redoes redone alone, the
    loop never."""
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    ones = counting(monkeypatch, matcher.ORBMatcher, "_fp_one")
    monkeypatch.setattr(matcher.ORBMatcher, "_local_loop", lambda *a: pytest.fail("the loop"))
    stats = {}
    want = LC.drive(golden, LC.by_oracle(stats), cfg)
    assert LC.same(want, LC.golden_results(golden, cfg))
    got = LC.drive(golden, LC.by_matcher(matcher.ORBMatcher), cfg)
    assert LC.same(got, want), LC.diff(got, want)
    assert [x[:2] for x in launches] == [(1, 1)] * LC.N_FRAMES
    assert sum(x[2] for x in launches) == stats["items"]
    redone = [(F.mnId - 40, p.mnId) for F, p, _ in ones]
    jobs, _ = LC.build(golden, LC.CONFIGS[cfg][0])
    assert redone == [(s, jobs[s][1][i].mnId) for s, i in stats["redone"]] and len(redone) > 0
    assert len(redone) < REDO_CAP * stats["items"]
    launches.clear(), ones.clear()
    got = LC.drive(golden, LC.by_matcher(matcher.ORBMatcher, many=True), cfg)
    assert LC.same(got, want), LC.diff(got, want)
    assert [x[:2] for x in launches] == [(LC.N_FRAMES, LC.N_FRAMES)] and len(ones) == len(redone)


def test_is_in_frustum_many_leaves_what_the_loop_leaves(golden):
    """Values, dtypes and shapes of every attribute, and the return values, against the reference's body point by
    point, for float32 and float64 poses, and for a list whose positions are not of one dtype (point by point)."""
    from pyorbslam_amd import frame as PF
    for dtype in (np.float32, np.float64):
        for mixed in (False, True):
            snaps = []
            for many in (False, True):
                jobs, w = LC.build(golden, dtype)
                if mixed:
                    for p in w.mps[::3]:
                        p._pos = p._pos.astype(np.float64 if dtype == np.float32 else np.float32)
                F, vp = jobs[0]
                if many:
                    seen = PF.is_in_frustum_many(F, vp, LC.LIMIT)
                else:
                    seen = [LO.frustum_one(F, p, LC.LIMIT) for p in vp]
                snaps.append((seen, LC.snapshot(w, jobs)))
            assert snaps[0][0] == snaps[1][0] and 20 < sum(snaps[0][0]) < len(snaps[0][0])
            assert all(type(x) is bool for x in snaps[1][0])
            for k, v in snaps[0][1].items():
                assert np.array_equal(v, snaps[1][1][k], equal_nan=(k == "val")), (dtype, mixed, k)
    assert PF.is_in_frustum_many(F, [], LC.LIMIT) == []


def test_is_in_frustum_many_follows_nan_comparisons():
    """pc.z == 0: 1 / 0 and the NaN comparisons after it decide as the reference's body does."""
    from pyorbslam_amd import frame as PF
    g = np.load(GOLDEN / "local_search.npz", allow_pickle=False)
    res = []
    for many in (False, True):
        jobs, w = LC.build(g, np.float64)
        F, vp = jobs[0]
        F.set_pose(np.eye(4))
        pts = vp[:6]
        for p, xyz in zip(pts, ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 5.0), (0.0, 0.0, -5.0),
                                (0.0, 0.0, 1e-300))):
            p._pos = np.array(xyz, np.float64).reshape(3, 1)
        seen = PF.is_in_frustum_many(F, pts, LC.LIMIT) if many else [LO.frustum_one(F, p, LC.LIMIT) for p in pts]
        res.append((seen, [bool(p.mbTrackInView) for p in pts]))
    assert res[0] == res[1]


FALLBACKS = ("no_device", "th_array", "th_inf", "limit_f32", "radius_overridden", "slots_tuple", "no_mbf", "f16_pose")


@pytest.mark.parametrize("name", FALLBACKS)
def test_every_fallback_reaches_the_loop(golden, monkeypatch, name):
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    loops = []
    monkeypatch.setattr(matcher.ORBMatcher, "_local_loop", lambda self, *a: loops.append(a) or (3, 2))
    jobs, _ = LC.build(golden, np.float64)
    F, vp = jobs[0]
    cls, th, limit = matcher.ORBMatcher, 1, 0.5
    if name == "no_device":
        monkeypatch.setattr(LIB, "device_present", lambda: False)
    elif name == "th_array":
        th = np.array([1.0])
    elif name == "th_inf":
        th = float("inf")
    elif name == "limit_f32":
        limit = np.float32(0.5)
    elif name == "radius_overridden":
        cls = type("M", (matcher.ORBMatcher,), {"radius_by_viewing_cos": lambda self, c: 3.0})
    elif name == "slots_tuple":
        F.mvpMapPoints = tuple(F.mvpMapPoints)
    elif name == "no_mbf":
        del F.mbf
    elif name == "f16_pose":
        F.mRcw = F.mRcw.astype(np.float16)
    assert cls(0.8, True).search_local_points(F, vp, th, limit) == (3, 2)
    assert len(loops) == 1 and not launches
    assert cls(0.8, True).search_local_points_many([F], [vp], th, limit) == [(3, 2)] and not launches


def test_many_with_a_repeated_frame_runs_the_loop(golden, monkeypatch):
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    jobs, _ = LC.build(golden, np.float64)
    F, vp = jobs[0]
    got = matcher.ORBMatcher(0.8, True).search_local_points_many([F, F], [vp, vp], 1)
    assert [x[:2] for x in launches] == [(1, 1), (1, 1)] and len(got) == 2
    with pytest.raises(ValueError):
        matcher.ORBMatcher(0.8, True).search_local_points_many([F], [vp, vp], 1)


def test_nothing_in_view_returns_none_and_a_point_the_arrays_cannot_express_goes_alone(golden, monkeypatch):
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    jobs, w = LC.build(golden, np.float64)
    F, vp = jobs[0]
    for p in vp:
        p.mnLastFrameSeen = F.mnId
    assert matcher.ORBMatcher(0.8, True).search_local_points(F, vp, 1) == (0, None) and not launches
    jobs, w = LC.build(golden, np.float64)
    ref, wr = LC.build(golden, np.float64)
    for ww in (w, wr):
        for p in ww.mps[::5]:
            p.mfMaxDistance = np.float16(p.mfMaxDistance)   # the arrays cannot express the point
        for p in ww.mps[1::5]:
            p.mfMaxDistance = np.float32(p.mfMaxDistance)   # widened exactly, as the reference's comparison does
    ones = counting(monkeypatch, matcher.ORBMatcher, "_fp_one")
    got = matcher.ORBMatcher(0.8, True).search_local_points(*jobs[0], 1)
    want = LO.loop(*ref[0], 1, LC.LIMIT, 0.8)
    assert got == want and launches[0][2] < len(jobs[0][1])
    a, b = LC.snapshot(w, jobs), LC.snapshot(wr, ref)
    assert all(np.array_equal(a[k], b[k], equal_nan=(k == "val")) for k in a)
    kinds = {type(p.mfMaxDistance) for _, p, _ in ones}
    sent = [p for p in jobs[0][1] if not LO.skipped(p, jobs[0][0]) and type(p.mfMaxDistance) is not np.float16]
    assert np.float16 in kinds and len(sent) == launches[0][2]
    assert any(type(p.mfMaxDistance) is np.float32 for p in sent)


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_new_symbols_resolve():
    L = LIB.lib()
    for name in NEW:
        assert name in LIB.SIGNATURES and getattr(L, name) is not None
    assert C.sizeof(LIB.LocalOut) == 7 * C.sizeof(C.c_void_p)
    assert L.orbfe_abi_version() == LIB.ORBFE_ABI_VERSION


def test_table_and_header_agree():
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(LIB.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_local_out \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in LIB.LocalOut._fields_] == list(LO.OUTPUTS)
    assert "orbfe_local_search" in hdr[:hdr.index("#define ORBFE_FRAME_RING")]   # named in the revision's comment
    src = ROOT / "pyorbslam_amd" / "csrc" / "orbfe_fuse.hip"
    assert re.search(r"^int orbfe_local_search\s*\(", src.read_text(), flags=re.M)


# ---- validation: everything is refused before the first device call -------------------------------------------------

REQUIRED = tuple(k for k in LO.ARRAYS if k != "blocked")


class HostCall:
    """orbfe_local_search over a small valid input (three frames, three searches, four items); each test breaks one
    thing."""

    def __init__(self):
        c = LC.by_name("two_limits_an_empty_frame_and_an_idle_one")
        self.a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in LC.arrays(c).items()}
        self.a["blocked"] = np.zeros(int(self.a["off"][-1]), np.uint8)
        self.n_kf, self.n_pts, self.n_srch, self.th, self.th_on, self.eps = 3, 2, 3, 1.0, 0, LO.EPS_F64
        self.o = {k: np.full(4, 7, np.uint8 if k in ("in_view", "status") else np.int32) for k in LO.OUTPUTS}
        self.null = set()

    def run(self):
        p = lambda k: None if k in self.null else LIB.ptr(self.a[k])  # noqa: E731
        out = LIB.LocalOut(**{k: None if k in self.null else v.ctypes.data for k, v in self.o.items()})
        rc = LIB.lib().orbfe_local_search(*[p(k) for k in LO.KF_ARRAYS], self.n_kf, p("pt_f64"), p("pt_desc"),
                                          self.n_pts, p("srch_limit"), p("srch_kf"), p("srch_off"), self.n_srch,
                                          p("item_pt"), self.th, self.th_on, self.eps,
                                          None if "out" in self.null else C.byref(out))
        return rc, LIB.lib().orbfe_last_error().decode()

    def untouched(self):
        return all(bool((x == 7).all()) for x in self.o.values())


def refused(h, *words):
    rc, msg = h.run()
    assert rc == LIB.ORBFE_EINVAL and all(w in msg for w in words), (rc, msg)
    assert "ORBFE_" not in msg and h.untouched()


@pytest.mark.parametrize("name", REQUIRED + ("out",) + LO.OUTPUTS)
def test_required_pointers(name):
    h = HostCall()
    h.null.add(name)
    refused(h, "null argument")


def test_search_checks():
    h = HostCall()
    h.a["srch_off"][0] = 1
    refused(h, "srch_off[0]", "must be 0")
    h = HostCall()
    h.a["srch_off"][1:] = [2, 1, 4]
    refused(h, "search 1", "must not decrease")
    for v in (3, -1):
        h = HostCall()
        h.a["srch_kf"][1] = v
        refused(h, "search 1", "outside the keyframes")
    for v in (2, -1):
        h = HostCall()
        h.a["item_pt"][2] = v
        refused(h, "item", "outside the point table")
    for v in (np.nan, np.inf, -np.inf):
        h = HostCall()
        h.a["srch_limit"][1] = v
        refused(h, "search 1", "limit", "finite")
        for col in range(9):                       # the normal included
            h = HostCall()
            h.a["pt_f64"][1, col] = v
            refused(h, "point scalar", "finite")
        for col in (0, 3, 4, 5, 13, 14, 16, 17, 19, 20, 23, 24, 26):   # bf included
            h = HostCall()
            h.a["kf_f64"][1, col] = v
            refused(h, "keyframe 1", "scalar", "finite")
        h = HostCall()
        h.a["u_right"][0] = v
        refused(h, "keyframe 0", "coordinate", "finite")
        h = HostCall()
        h.eps = v
        refused(h, "th and eps")
    for kw in (dict(n_kf=-1), dict(n_pts=-1), dict(n_srch=-1), dict(n_kf=65536)):
        h = HostCall()
        for k, v in kw.items():
            setattr(h, k, v)
        assert h.run()[0] == LIB.ORBFE_EINVAL and h.untouched()


def test_the_frame_checks_are_the_other_entries():
    h = HostCall()
    h.a["kf_i32"][1, 0] = 0
    refused(h, "keyframe 1", "columns and rows")
    h = HostCall()
    h.a["cell_off"][0] = 1
    refused(h, "keyframe 0", "first cell offset")
    h = HostCall()
    h.a["octave"][0] = 4
    refused(h, "keyframe 0", "octave")
    h = HostCall()
    h.a["cell_idx"][0] = 1
    refused(h, "keyframe 0", "grid entry", "outside")


def test_nothing_to_do_needs_no_device():
    h = HostCall()
    h.null.add("blocked")
    assert h.run()[0] != LIB.ORBFE_EINVAL
    h = HostCall()
    h.a["srch_off"][:] = 0
    assert h.run()[0] == 0 and h.untouched()
    h = HostCall()
    h.n_srch = 0
    assert h.run()[0] == 0 and h.untouched()
    h = HostCall()
    h.n_srch, h.null = 0, set(LO.ARRAYS) | {"out"}
    assert h.run()[0] == 0
    from pyorbslam_amd import matcher
    a = LC.arrays(LC.by_name("zero_searches"))
    out = matcher.local_search_arrays(*[a[k] for k in LO.ARRAYS], a["th"], a["th_on"], a["eps"])
    assert list(out) == list(LO.OUTPUTS) and all(len(v) == 0 for v in out.values())


# ---- the C3 tracking loop's first frames -----------------------------------------------------------------------------

def c3_scenes(extractors, frame_cls):
    import json

    import local_search_seq as LS
    import seq_harness as H
    from pyorbslam_amd import synth
    g = H.load_golden()
    meta = json.loads(str(g["meta"]))
    seq = synth.StereoSequence(meta["seq"]["seed"], meta["width"], meta["height"], meta["seq"]["speed"])
    return g, meta["proj_kinds"], LS.scenes(g, seq, extractors, frame_cls)


def check_c3(monkeypatch, matcher, scenes, g, kinds, launches, ones):
    """Per frame: is_in_frustum_many alone against the recorded projections; the oracle's replay against the recorded
    search; then search_local_points from the frame's state before either, against both records, with one launch and
    exactly the replay's redos.  Frame 1 is predicted with frame 0's own pose: every point is as far from the camera
    as when it was made, its level quotient is an integer and the item is marked, so the cap is asked of frames 2 and
    3 only."""
    import local_search_seq as LS
    from pyorbslam_amd import frame as PF
    shares = {}
    for k, cur, local in scenes:
        before = list(cur.mvpMapPoints)

        def reset():
            cur.mvpMapPoints[:] = before
            for q in local:
                q.mbTrackInView = False
        seen = PF.is_in_frustum_many(cur, [q for q in local if q.mnLastFrameSeen != cur.mnId], LC.LIMIT)
        assert sum(seen) == len(g[f"f{k}_local_ids"]) > 100 and LS.frustum_differs(g, k, local, kinds) == []
        reset()
        stats = {}
        res = LO.replay([(cur, local)], 1, LC.LIMIT, 0.8, stats=stats)[0]
        assert LS.search_differs(g, k, cur, res) == [] and LS.frustum_differs(g, k, local, kinds) == []
        reset()
        launches.clear(), ones.clear()
        res = matcher.ORBMatcher(0.8, True).search_local_points(cur, local, 1)
        assert LS.search_differs(g, k, cur, res) == [] and LS.frustum_differs(g, k, local, kinds) == []
        assert len(launches) == 1 and [p.mp_id for p in ones] == [local[i].mp_id for _, i in stats["redone"]]
        shares[k] = (len(ones), stats["items"])
    assert sorted(shares) == [1, 2, 3]
    for k in (2, 3):
        assert 0 < shares[k][0] < REDO_CAP * shares[k][1], shares
    return shares


def test_c3_frames_through_the_oracle(monkeypatch):
    """Frames 1-3 of the C3 golden through the oracle extraction, with the array oracle in the kernel's place."""
    from pyorbslam_amd import matcher
    from test_sequence import _OracleExtractor, _OracleFrame
    import seq_harness as H
    launches, ones = [], []
    fake_device(monkeypatch, matcher, launches)
    inner = matcher.ORBMatcher._fp_one
    monkeypatch.setattr(matcher.ORBMatcher, "_fp_one", lambda self, F, p, th: ones.append(p) or inner(self, F, p, th))
    monkeypatch.setattr(matcher.ORBMatcher, "_local_loop", lambda *a: pytest.fail("the loop"))
    g, kinds, scenes = c3_scenes((_OracleExtractor(**H.PARAMS), _OracleExtractor(**H.PARAMS)), _OracleFrame)
    shares = check_c3(monkeypatch, matcher, scenes, g, kinds, launches, ones)
    assert shares[1][0] == shares[1][1]   # the finding: every item of frame 1 is marked
