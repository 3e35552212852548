"""k_fkf_search without a device: the placed cases against the array oracle, the oracle against the reference's
golden, the product's packing, prefilter and replay with the oracle in the kernel's place, the fallbacks, the ABI and
every validation path of orbfe_fkf_search (all of which return before the first device call)."""
import ctypes as C
import re

import numpy as np
import pytest

import fkf_cases as KC
import fkf_oracle as FK
import matcher_world as MW
from conftest import GOLDEN, ROOT
from pyorbslam_amd import _lib as LIB

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")
NEW = ("orbfe_fkf_search", "orbfe_fkf_search_last_ms")

CASES = KC.all_cases()
ORACLE = {c["name"]: KC.oracle(c) for c in CASES}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "fkf.npz", allow_pickle=False)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_holds_its_claim(case):
    bi, bd, st = ORACLE[case["name"]]
    case["check"](bi, bd, st)
    assert np.flatnonzero(st).tolist() == case["marked"]
    assert bi.dtype == bd.dtype == np.int32 and st.dtype == np.uint8 and len(bi) == sum(map(len, case["items"]))


def _differs(name, **switch):
    a, b = ORACLE[name], KC.oracle(KC.by_name(name), **switch)
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_the_set_is_not_vacuous():
    """Each property of the mode, turned off in the oracle, changes the answer of the case built for it."""
    assert _differs("behind_the_camera_is_searched_and_depth_zero_marked", depth_gate=True)
    assert _differs("u_on_max_x_is_inside_and_marked", exclusive_max=True)
    assert _differs("upper_end_truncates", floor_ceil=True)
    assert _differs("octave_one_above_the_level_wins", two_octaves=True)
    assert _differs("normal_slots_hold_nan_and_no_viewing_gate", viewing_gate=True)
    assert _differs("closest_candidate_blocked", blocked=False) and _differs("every_candidate_blocked", blocked=False)
    for name in ("tie_in_two_cells", "tie_in_one_unsorted_cell", "window_65"):
        assert _differs(name, early_tie=False)
    sizes = [len(it) for it in KC.by_name("ragged_0_1_255_256_257")["items"]]
    assert sizes == [1, 0, 255, 256, 0, 257, 0]
    marked = [c["name"] for c in CASES if c["marked"]]
    assert marked == ["behind_the_camera_is_searched_and_depth_zero_marked", "u_on_max_x_is_inside_and_marked",
                      "v_on_min_y_is_inside_and_marked", "distance_on_min_and_max_marked_outside_skipped",
                      "eps_of_float32_marks_what_float64_does_not"]


# ---- the golden ------------------------------------------------------------------------------------------------------

def test_oracle_and_replay_reproduce_the_reference(golden):
    """Every search of every configuration: the oracle with its redo gives the reference's n and slots, every
    unmarked item decides as the reference's loop body, at most 2 % of the items that reach a window are marked, and
    the events the file was chosen for are there."""
    stats = {}
    most = 0
    for cfg in range(len(KC.CONFIGS)):
        got = KC.drive(golden, KC.by_oracle(stats, agree=True), cfg)
        assert KC.same(got, KC.golden_results(golden, cfg)), cfg
        most = max(most, max(got[0]))
    assert most >= 20 and stats["taken"] > 0 and stats["rotated"] > 0 and stats["behind"] > 0 and stats["stable"]
    assert 0 < stats["marginal"] <= 0.02 * stats["reached"]
    w = MW.build(golden)
    jobs = KC.jobs_of(w, golden)
    assert all(len(found) > 0 for _, _, found in jobs)
    filled = sum(p is not None for p in jobs[0][0].mvpMapPoints)
    assert abs(filled - jobs[0][0].N // 4) <= 1 and golden["kf0_T"].dtype == np.float32


@pytest.mark.parametrize("seed", [51, 52, 53])
def test_unmarked_items_decide_as_the_reference_and_few_are_marked(seed):
    """The soundness of the bound on random float32 worlds, in the golden's configurations: wherever the oracle leaves
    the status 0, its winner and distance are those of the reference's loop body on the objects.  At most 2 % of the
    items that reach a cell window may be marked."""
    import fuse_cases as FC
    g = FC.Z(KC.make_extras(FC.clone_world(seed), seed))
    stats = {}
    for cfg in range(len(KC.CONFIGS)):
        KC.drive(g, KC.by_oracle(stats, agree=True), cfg)
    reached, marked = stats["reached"], stats["marginal"]
    print(f"items {stats['items']} reached {reached} marked {marked} share {marked / reached:.4f}")
    assert reached > 1000
    assert marked <= 0.02 * reached


# ---- the product with the oracle in the kernel's place ---------------------------------------------------------------

def fake_device(monkeypatch, matcher, launches):
    def arrays(*args):
        a = dict(zip(FK.ARRAYS + ("th", "eps"), args))
        launches.append((len(a["kf_f64"]), len(a["srch_kf"]), int(a["srch_off"][-1])))
        bi, bd, st = FK.search(a)
        return dict(best_idx=bi, best_dist=bd, status=st)
    monkeypatch.setattr(LIB, "device_present", lambda: True)
    monkeypatch.setattr(matcher, "fkf_search_arrays", arrays)


def counting(monkeypatch, cls, name):
    calls, inner = [], getattr(cls, name)

    def wrapped(self, *a, **k):
        calls.append(a)
        return inner(self, *a, **k)
    monkeypatch.setattr(cls, name, wrapped)
    return calls


@pytest.mark.parametrize("cfg", range(len(KC.CONFIGS)))
def test_device_path_replays_the_reference(golden, monkeypatch, cfg):
    """search_by_projection_f_kf_f and _many over the oracle's arrays: the golden's n and slots, one launch per call
    (one for all six searches of _many), exactly the marked and the overtaken items redone, the host body never."""
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    ones = counting(monkeypatch, matcher.ORBMatcher, "_fkf_one")
    monkeypatch.setattr(matcher.ORBMatcher, "_fkf_host", lambda *a: pytest.fail("host body"))
    stats = {}
    want = KC.drive(golden, KC.by_oracle(stats), cfg)
    assert KC.same(want, KC.golden_results(golden, cfg))
    got = KC.drive(golden, KC.loop_single(matcher.ORBMatcher), cfg)
    assert KC.same(got, want) and all(type(n) is int for n in got[0])
    assert [x[:2] for x in launches] == [(1, 1)] * KC.N_SEARCH and len(ones) == stats["redone"] > 0
    launches.clear(), ones.clear()
    got = KC.drive(golden, KC.many(matcher.ORBMatcher), cfg)
    assert KC.same(got, want)
    assert [x[:2] for x in launches] == [(KC.N_SEARCH, KC.N_SEARCH)] and len(ones) == stats["redone"]


def test_host_body_reproduces_the_reference(golden, monkeypatch):
    """The former body of the public method, moved to _fkf_host, with the Hamming distances on the host."""
    from pyorbslam_amd import matcher
    from test_matcher_kf import _cpu_batched
    monkeypatch.setattr(matcher.ORBMatcher, "_batched", staticmethod(_cpu_batched))
    for cfg in (1, 3):
        got = KC.drive(golden, KC.loop_single(matcher.ORBMatcher, "_fkf_host"), cfg)
        assert KC.same(got, KC.golden_results(golden, cfg))


def _fresh(golden, k=0):
    w = MW.build(golden)
    return w, KC.jobs_of(w, golden)[k]


FALLBACKS = {
    "th_is_float32": lambda F, a: a.update(th=np.float32(10.0)),
    "th_is_nan": lambda F, a: a.update(th=float("nan")),
    "orbdist_is_256": lambda F, a: a.update(orb=256),
    "orbdist_is_numpy_int": lambda F, a: a.update(orb=np.int64(100)),
    "orbdist_is_nan": lambda F, a: a.update(orb=float("nan")),
    "slots_are_a_tuple": lambda F, a: setattr(F, "mvpMapPoints", tuple(F.mvpMapPoints)),
    "slots_are_one_short": lambda F, a: F.mvpMapPoints.pop(),
    "no_frame_grid_cols": lambda F, a: delattr(F, "FRAME_GRID_COLS"),
    "grid_rows_do_not_fit": lambda F, a: setattr(F, "FRAME_GRID_ROWS", F.FRAME_GRID_ROWS - 1),
    "pose_is_float16": lambda F, a: setattr(F, "mTcw", F.mTcw.astype(np.float16)),
    "pose_is_not_finite": lambda F, a: F.mTcw.__setitem__((0, 3), np.inf),
    "pose_is_3x4": lambda F, a: setattr(F, "mTcw", F.mTcw[:3]),
    "fx_is_float32": lambda F, a: setattr(F, "fx", np.float32(F.fx)),
    "min_x_is_an_int": lambda F, a: setattr(F, "mnMinX", 0),
    "level_count_is_a_float": lambda F, a: setattr(F, "mnScaleLevels", 8.0),
    "scale_table_is_short": lambda F, a: setattr(F, "mvScaleFactors", F.mvScaleFactors[:5]),
    "descriptors_are_a_list": lambda F, a: setattr(F, "mDescriptors", list(F.mDescriptors)),
}


@pytest.mark.parametrize("name", ["no_device"] + list(FALLBACKS))
def test_every_fallback_reaches_the_host_body(golden, monkeypatch, name):
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    if name == "no_device":
        monkeypatch.setattr(LIB, "device_present", lambda: False)
    hosts = []
    monkeypatch.setattr(matcher.ORBMatcher, "_fkf_host", lambda self, *a: hosts.append(a) or 7)
    w, (F, kf, found) = _fresh(golden)
    a = dict(th=10.0, orb=100)
    if name != "no_device":
        FALLBACKS[name](F, a)
    m = matcher.ORBMatcher()
    assert m.search_by_projection_f_kf_f(F, kf, found, a["th"], a["orb"]) == 7
    assert len(hosts) == 1 and hosts[0][0] is F and hosts[0][1] is kf and hosts[0][2] is found and not launches
    assert m.search_by_projection_f_kf_f_many([F], [kf], [found], a["th"], a["orb"]) == [7]
    assert len(hosts) == 2 and not launches


def test_plain_int_th_and_float_orbdist_take_the_device_path(golden, monkeypatch):
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    monkeypatch.setattr(matcher.ORBMatcher, "_fkf_host", lambda *a: pytest.fail("host body"))
    w, (F, kf, found) = _fresh(golden)
    n = matcher.ORBMatcher().search_by_projection_f_kf_f(F, kf, found, 10, 100.0)
    assert n == int(golden["fkf_n0"][0]) and len(launches) == 1


def test_a_point_the_arrays_cannot_express_goes_alone(golden, monkeypatch):
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    ones = counting(monkeypatch, matcher.ORBMatcher, "_fkf_one")
    stats = {}
    want = KC.drive(golden, KC.by_oracle(stats), 0)
    w = MW.build(golden)
    jobs = KC.jobs_of(w, golden)[:1]
    odd = [p for p in jobs[0][1].mvpMapPoints if p and not p.is_bad() and p not in jobs[0][2]][:3]
    for p in odd:
        p.mfMaxDistance = np.float32(p.mfMaxDistance)
    for p in w.mps:
        p.get_normal = None   # the reference never asks for the normal
    with np.errstate(all="ignore"):
        n = matcher.ORBMatcher().search_by_projection_f_kf_f(*jobs[0], 10.0, 100)
    assert len(launches) == 1 and all(any(c[1] is p for c in ones) for p in odd)
    # float32(mfMaxDistance) moves no level here: the result is the golden's
    assert n == want[0][0] and np.array_equal(MW.encode_mps(w, jobs[0][0].mvpMapPoints), want[1][0])


def test_many_with_a_repeated_frame_runs_the_loop(golden, monkeypatch):
    """The same frame against two keyframes: the second search reads what the first assigned, so _many is the loop of
    single calls, launch for launch and slot for slot; a length mismatch is refused."""
    from pyorbslam_amd import matcher
    launches = []
    fake_device(monkeypatch, matcher, launches)
    outs = []
    for use_many in (False, True):
        w = MW.build(golden)
        jobs = KC.jobs_of(w, golden)
        F = jobs[0][0]
        args = ([F, jobs[2][0], F], [jobs[0][1], jobs[2][1], jobs[1][1]], [jobs[0][2], jobs[2][2], jobs[1][2]])
        m = matcher.ORBMatcher()
        launches.clear()
        if use_many:
            ns = m.search_by_projection_f_kf_f_many(*args, 10.0, 100)
        else:
            ns = [m.search_by_projection_f_kf_f(*j, 10.0, 100) for j in zip(*args)]
        assert [x[:2] for x in launches] == [(1, 1)] * 3
        outs.append((ns, MW.encode_mps(w, F.mvpMapPoints), MW.encode_mps(w, jobs[2][0].mvpMapPoints)))
    assert outs[0][0] == outs[1][0] and all(np.array_equal(a, b) for a, b in zip(outs[0][1:], outs[1][1:]))
    assert outs[0][0][2] < int(golden["fkf_n0"][1])   # the second visit finds slots taken
    with pytest.raises(ValueError):
        matcher.ORBMatcher().search_by_projection_f_kf_f_many([F], [], [], 10.0, 100)
    assert matcher.ORBMatcher().search_by_projection_f_kf_f_many([], [], [], 10.0, 100) == []


def test_redo_raises_what_the_reference_raises(golden, monkeypatch):
    """A point on the frame's camera centre, with no minimum distance: the reference's u and v are NaN and pass its
    four comparisons, the distance is 0, the level quotient is infinite and its int() raises.  The item comes back
    marked and the redo raises the same."""
    from pyorbslam_amd import matcher
    fake_device(monkeypatch, matcher, [])
    w, (F, kf, found) = _fresh(golden)
    p = next(q for q in kf.mvpMapPoints if q and not q.is_bad() and q not in found)
    F.mTcw = np.eye(4)
    F.Tcw = F.mTcw
    p._pos = np.zeros((3, 1))
    p.mfMinDistance = 0.0
    with pytest.raises((ValueError, OverflowError)) as mine, np.errstate(all="ignore"):
        matcher.ORBMatcher().search_by_projection_f_kf_f(F, kf, found, 10.0, 100)
    with pytest.raises((ValueError, OverflowError)) as ref, np.errstate(all="ignore"):
        FK.single_item(F, p, 10.0)
    assert type(mine.value) is type(ref.value) and str(mine.value) == str(ref.value)


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_new_symbols_resolve():
    L = LIB.lib()
    for name in NEW:
        assert name in LIB.SIGNATURES and getattr(L, name) is not None
    assert C.sizeof(LIB.FkfOut) == 3 * C.sizeof(C.c_void_p)
    assert L.orbfe_abi_version() == LIB.ORBFE_ABI_VERSION


def test_table_and_header_agree():
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        m = re.search(r"^int " + name + r"\s*\((.*?)\);", code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(LIB.SIGNATURES[name]), name
    fields = re.search(r"typedef struct orbfe_fkf_out \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in LIB.FkfOut._fields_]
    assert int(re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1)) == LIB.ORBFE_ABI_VERSION
    assert "orbfe_fkf_search" in hdr[:hdr.index("#define ORBFE_FRAME_RING")]   # named in the revision's comment
    src = ROOT / "pyorbslam_amd" / "csrc" / "orbfe_fuse.hip"
    assert re.search(r"^int orbfe_fkf_search\s*\(", src.read_text(), flags=re.M)


# ---- validation: everything is refused before the first device call -------------------------------------------------

OUTS = ("best_idx", "best_dist", "status")
REQUIRED = tuple(k for k in FK.ARRAYS if k != "blocked")


class HostCall:
    """orbfe_fkf_search over a small valid input (four frames, three searches, four items); each test breaks one
    thing."""

    def __init__(self):
        c = KC.by_name("four_frames_two_grids_one_empty_one_idle")
        self.a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in KC.arrays(c).items()}
        self.a["blocked"] = np.zeros(int(self.a["off"][-1]), np.uint8)
        self.n_kf, self.n_pts, self.n_srch, self.th, self.eps = 4, 2, 3, KC.TH, FK.EPS_F64
        self.o = dict(best_idx=np.full(4, -7, np.int32), best_dist=np.full(4, -7, np.int32),
                      status=np.full(4, 7, np.uint8))
        self.null = set()

    def run(self):
        p = lambda k: None if k in self.null else LIB.ptr(self.a[k])  # noqa: E731
        out = LIB.FkfOut(**{k: None if k in self.null else v.ctypes.data for k, v in self.o.items()})
        rc = LIB.lib().orbfe_fkf_search(*[p(k) for k in FK.KF_ARRAYS], self.n_kf, p("pt_f64"), p("pt_desc"), self.n_pts,
                                        p("srch_kf"), p("srch_off"), self.n_srch, p("item_pt"), self.th, self.eps,
                                        None if "out" in self.null else C.byref(out))
        return rc, LIB.lib().orbfe_last_error().decode()

    def untouched(self):
        return all(bool((x == (7 if k == "status" else -7)).all()) for k, x in self.o.items())


def refused(h, *words):
    rc, msg = h.run()
    assert rc == LIB.ORBFE_EINVAL and all(w in msg for w in words), (rc, msg)
    assert "ORBFE_" not in msg and h.untouched()


@pytest.mark.parametrize("name", REQUIRED + ("out",) + OUTS)
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
    for v in (4, -1):
        h = HostCall()
        h.a["srch_kf"][1] = v
        refused(h, "search 1", "outside the keyframes")
    for v in (2, -1):
        h = HostCall()
        h.a["item_pt"][2] = v
        refused(h, "item", "outside the point table")
    for v in (np.nan, np.inf, -np.inf):
        for col in (0, 2, 6, 7, 8):
            h = HostCall()
            h.a["pt_f64"][1, col] = v
            refused(h, "point scalar", "finite")
        for col in (0, 3, 5, 13, 14, 16, 17, 19, 20, 23, 24, 26):
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


def test_the_frame_checks_are_the_other_entries():
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
    h = HostCall()
    n = LIB.ORBFE_BOW_MAX_FRAME + 1
    h.a["off"][1:] += n
    h.a["xy"] = np.zeros((int(h.a["off"][-1]), 2))
    refused(h, "keyframe 0", "limit")


def test_slots_that_are_not_read_are_not_checked_and_nothing_to_do_needs_no_device():
    """Non-finite values in the slots the mode does not read (bf, the normal) pass the validation, and blocked may be
    null (what follows needs a device and is tests/test_gpu_fkf.py's); with no item to search the call returns
    before any device call."""
    h = HostCall()
    h.a["kf_f64"][:, 4] = np.nan
    h.a["pt_f64"][:, 3:6] = np.inf
    h.null.add("blocked")
    assert h.run()[0] != LIB.ORBFE_EINVAL
    h = HostCall()
    h.a["srch_off"][:] = 0
    assert h.run()[0] == 0 and h.untouched()
    h = HostCall()
    h.n_srch = 0
    assert h.run()[0] == 0 and h.untouched()
    h = HostCall()
    h.n_srch, h.null = 0, set(FK.ARRAYS) | {"out"}
    assert h.run()[0] == 0
