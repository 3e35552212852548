"""The five projection search kernels on the flip-point ladders of tests/margin_cases.py: one launch per mode and
precision over all of its ladders, every output bit for bit the array oracle's, status included.  A rung is marked
where the oracle marks it and nowhere else, so the rung at which a ladder's mark disappears pins the size of each
bound to a factor of two on the device itself: a `2.0 * rz` compiled as `rz`, or a dropped `4.0 * eps * Mu`, moves
that rung."""
import numpy as np
import pytest

import fkf_oracle as FK
import fuse_cases as FC
import fuse_oracle as O
import local_search_cases as LC
import local_search_oracle as LO
import margin_cases as M
import scw_oracle as SO
import sim3_oracle as S3

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]

SETS = [(m, p) for m in M.MODES for p in M.PRECISIONS]
IDS = [f"{m}-{p}" for m, p in SETS]
ARRAYS = {"fuse": O.ARRAYS, "scw": SO.ARRAYS, "sim3": S3.ARRAYS, "fkf": FK.ARRAYS, "local": LO.ARRAYS}
OUTPUTS = ("best_idx", "best_dist", "status")


def run_host(mode, a):
    from pyorbslam_amd import matcher
    entry = getattr(matcher, f"{mode}_search_arrays")
    args = [a[k] for k in ARRAYS[mode]] + ([a["th"], a["th_on"], a["eps"]] if mode == "local" else [a["th"], a["eps"]])
    r = entry(*args)
    return [r[k] for k in (LO.OUTPUTS if mode == "local" else OUTPUTS)]


@pytest.mark.parametrize("mode,prec", SETS, ids=IDS)
def test_the_kernel_marks_and_decides_every_rung_as_the_oracle(mode, prec):
    S = M.get(mode, prec)
    items, left_out = M.device_rungs(S)
    assert len(items) >= 2 * (M.J + 1) * len(S.ladders) - len(left_out) > 1000
    a, at = S.arrays(items)
    want = S.search(a)
    got = run_host(mode, a)
    names = LO.OUTPUTS if mode == "local" else OUTPUTS
    where = {i: n for n, i in enumerate(at)}
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        told = []
        for i in bad[:5].tolist():     # which rung of which ladder (a dense mode also has every point in the other target)
            n = where.get(i)
            lad = S.ladders[items[n][0]] if n is not None else None
            told.append((i, int(g.reshape(-1)[i]), int(w.reshape(-1)[i])) + (
                (lad["gate"], lad["sub"], lad["start"].i, items[n][1]) if lad else ("other target",)))
        assert not len(bad), (name, len(bad), told)
    # the marks are there to be compared: every ladder's innermost rungs that went to the device are marked, and the
    # outermost are not
    st = want[-1].reshape(-1)
    marked = sum(int(st[at[n]] != 0) for n in range(len(items)))
    assert marked >= 2 * len(S.ladders) - len(left_out) and marked < len(items) - 2 * 0.9 * len(S.ladders)


# ---- the public calls on the ladders --------------------------------------------------------------------------------
# One float32 ladder set per mode through the public call, on a world of its own (the calls write into it).  Three
# runs: the public call; the oracle's replay over the device's own results, which tells which items have to be redone
# alone; and the same replay with every item marked, which is the loop of reference bodies.  All three leave the same
# world behind, and the public call redoes alone exactly the items the replay redoes: the marked ones, and those an
# earlier item of the call has overtaken.

INNER = 8   # the rungs up to +-2^8: in float32 every ladder's mark ends by 2^7 (DESIGN.md's table)


def worlds_of(mode):
    """Three equal worlds, built before anything is recorded (building one runs the reference bodies)."""
    return iter([world_of(mode) for _ in range(3)])


def world_of(mode):
    S = M.Set(mode, "f32")
    items = [it for it in S.items() if abs(it[1]) <= 1 << INNER]
    pts = [it[3] for it in items]
    S.world.kfs, S.world.mps = list(S.targets), pts
    return S, [[p for it, p in zip(items, pts) if it[2] == k] for k in range(2)], pts


def keep_results(monkeypatch, matcher, mode, names):
    kept, arrays = [], getattr(matcher, f"{mode}_search_arrays")
    monkeypatch.setattr(matcher, f"{mode}_search_arrays", lambda *a, **k: kept.append(arrays(*a, **k)) or kept[-1])
    return kept, lambda: tuple(np.concatenate([r[k] for r in kept]) for k in names)


def recorded(monkeypatch, owner, name, key):
    calls, inner = [], getattr(owner, name)
    monkeypatch.setattr(owner, name, lambda *a, **k: calls.append(key(*a)) or inner(*a, **k))
    return calls


def all_marked(dev):
    return tuple(np.ones_like(x) if n == len(dev) - 1 else np.full_like(x, 0 if x.dtype == np.uint8 else -1)
                 for n, x in enumerate(dev))


def slots_of(targets):
    return [[p.mnId if p else -1 for p in t.mvpMapPoints] for t in targets]


def test_fuse_pkf_mp_many_on_the_ladders(monkeypatch):
    from pyorbslam_amd import matcher
    worlds = worlds_of("fuse")
    S, _, pts = next(worlds)
    m = matcher.ORBMatcher()
    kept, _ = keep_results(monkeypatch, matcher, "fuse", OUTPUTS)
    singles = recorded(monkeypatch, m, "_fuse_one", lambda kf, p, *a: (kf.mnId, p.mnId))
    got = FC.world_state(S.world, m.fuse_pkf_mp_many(S.targets, pts, S.th))
    assert len(kept) == 1
    dev = tuple(kept[0][k] for k in OUTPUTS)
    redone = recorded(monkeypatch, O, "single_item", lambda kf, p, *a: (kf.mnId, p.mnId))
    S, _, pts = next(worlds)
    replay = FC.world_state(S.world, O.replay(S.targets, pts, S.th, results=dev))
    want = list(redone)
    S, _, pts = next(worlds)
    loop = FC.world_state(S.world, O.replay(S.targets, pts, S.th, results=all_marked(dev)))
    FC.assert_state(replay, loop, "the replay against the loop of reference bodies")
    FC.assert_state(got, loop, "the public call against the loop of reference bodies")
    assert len(want) > 100 and int(loop["ret"].sum()) > 20, (len(want), loop["ret"])
    assert singles == want


def test_fuse_kf_scw_mp_many_on_the_ladders(monkeypatch):
    from pyorbslam_amd import matcher
    worlds = worlds_of("scw")

    def state(S, res):
        d = FC.world_state(S.world, [r[0] for r in res])
        d["rep"] = np.array([[q.mnId if q else -1 for q in r[1]] for r in res], np.int32)
        return d
    S, _, pts = next(worlds)
    Scws = [c["Scw"] for c in S.ctx]
    m = matcher.ORBMatcher()
    kept, _ = keep_results(monkeypatch, matcher, "scw", OUTPUTS)
    singles = recorded(monkeypatch, m, "_scw_one", lambda kf, p, *a: (kf.mnId, p.mnId))
    got = state(S, m.fuse_kf_scw_mp_many(S.targets, Scws, pts, S.th))
    assert len(kept) == 1
    dev = tuple(kept[0][k] for k in OUTPUTS)
    redone = recorded(monkeypatch, SO, "single_item", lambda kf, p, *a: (kf.mnId, p.mnId))
    S, _, pts = next(worlds)
    replay = state(S, SO.replay_fuse(S.targets, Scws, pts, S.th, results=dev))
    want = list(redone)
    S, _, pts = next(worlds)
    loop = state(S, SO.replay_fuse(S.targets, Scws, pts, S.th, results=all_marked(dev)))
    for k in loop:
        assert np.array_equal(replay[k], loop[k]) and np.array_equal(got[k], loop[k]), k
    assert singles == want and len(want) > 100 and int(loop["ret"].sum()) > 20


class Holder:
    """The keyframe of search_by_projection_f_kf_f as far as the search reads it: a list of map points."""

    def __init__(self, pts):
        self.pts = pts

    def get_map_point_matches(self):
        return list(self.pts)


def test_search_by_projection_f_kf_f_on_the_ladders(monkeypatch):
    from pyorbslam_amd import matcher
    worlds = worlds_of("fkf")
    S, lists, _ = next(worlds)
    jobs = [(F, Holder(vp), set()) for F, vp in zip(S.targets, lists)]
    m = matcher.ORBMatcher(1, False)
    kept, dev_of = keep_results(monkeypatch, matcher, "fkf", OUTPUTS)
    singles = recorded(monkeypatch, matcher.ORBMatcher, "_fkf_one", lambda self, F, p, *a: p.mnId)
    got = [m.search_by_projection_f_kf_f(F, kf, found, S.th, 100) for F, kf, found in jobs], slots_of(S.targets)
    assert len(kept) == 2
    dev = dev_of()
    redone = recorded(monkeypatch, FK, "single_item", lambda F, p, *a: p.mnId)
    S, lists, _ = next(worlds)
    jobs = [(F, Holder(vp), set()) for F, vp in zip(S.targets, lists)]
    replay = FK.replay(jobs, S.th, 100, False, results=dev), slots_of(S.targets)
    want = list(redone)
    S, lists, _ = next(worlds)
    jobs = [(F, Holder(vp), set()) for F, vp in zip(S.targets, lists)]
    loop = FK.replay(jobs, S.th, 100, False, results=all_marked(dev)), slots_of(S.targets)
    assert replay == loop and got == loop
    assert singles == want and len(want) > 100 and sum(loop[0]) > 20


def test_search_local_points_on_the_ladders(monkeypatch):
    from pyorbslam_amd import matcher
    worlds = worlds_of("local")
    nn = 0.8

    def same(a, b):
        return a[0] == b[0] and all(np.array_equal(a[1][k], b[1][k], equal_nan=(k == "val")) for k in b[1])
    S, lists, _ = next(worlds)
    jobs = list(zip(S.targets, lists))
    m = matcher.ORBMatcher(nn, True)
    kept, dev_of = keep_results(monkeypatch, matcher, "local", LO.OUTPUTS)
    singles = recorded(monkeypatch, matcher.ORBMatcher, "_fp_one", lambda self, F, p, *a: (F.mnId - 40, p.mnId))
    got = [m.search_local_points(F, vp, S.th, M.LIMIT) for F, vp in jobs], LC.snapshot(S.world, jobs)
    assert len(kept) == 2
    dev = dev_of()
    S, lists, _ = next(worlds)
    jobs = list(zip(S.targets, lists))
    stats = {}
    replay = LO.replay(jobs, S.th, M.LIMIT, nn, results=dev, stats=stats), LC.snapshot(S.world, jobs)
    want = [(s, jobs[s][1][i].mnId) for s, i in stats["redone"]]
    S, lists, _ = next(worlds)
    jobs = list(zip(S.targets, lists))
    loop = LO.replay(jobs, S.th, M.LIMIT, nn, results=all_marked(dev)), LC.snapshot(S.world, jobs)
    assert same(replay, loop) and same(got, loop)
    assert singles == want and len(want) > 100 and sum(n for _, n in loop[0]) > 20


def test_search_by_sim3_on_the_ladders(monkeypatch):
    """Each target's ladders are pKF1's map points (direction 1); the target holds none, so direction 2 is empty and
    the mutual check refuses every winner: what is compared is which items were redone alone, and that nothing is
    matched."""
    from pyorbslam_amd import matcher
    worlds = worlds_of("sim3")

    def pairs_of(S, lists):
        return [(S.first_keyframe(k, lists[k]), [(S.targets[k], [None] * len(lists[k]), c["s12"], c["R12"], c["t12"])])
                for k, c in enumerate(S.ctx)]

    def state(res):
        return [(n, [p.mnId if p else -1 for p in vm]) for n, vm in res]
    S, lists, _ = next(worlds)
    m = matcher.ORBMatcher()
    kept, dev_of = keep_results(monkeypatch, matcher, "sim3", OUTPUTS)
    singles = recorded(monkeypatch, m, "_sim3_one", lambda p, *a: p.mnId)
    monkeypatch.setattr(m, "_sim3_host", lambda *a: pytest.fail("host body"))
    got = state([m.search_by_sim3(kf1, *pr[0], S.th) for kf1, pr in pairs_of(S, lists)])
    assert len(kept) == 2
    dev = [tuple(r[k] for k in OUTPUTS) for r in kept]
    redone = recorded(monkeypatch, S3, "single_item", lambda p, *a: p.mnId)
    S, lists, _ = next(worlds)
    stats = {}
    replay = state([S3.replay(kf1, pr, S.th, results=d, stats=stats)[0] for (kf1, pr), d in zip(pairs_of(S, lists), dev)])
    want = list(redone)
    S, lists, _ = next(worlds)
    loop = state([S3.replay(kf1, pr, S.th, results=all_marked(d))[0] for (kf1, pr), d in zip(pairs_of(S, lists), dev)])
    assert replay == loop and got == loop
    assert singles == want and len(want) > 100 and stats["refused"] > 100
