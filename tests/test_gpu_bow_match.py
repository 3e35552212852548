"""k_bow_match on the GPU: the host entry on every crafted case against the array oracle, the device entry's
bounds, flags and strides, the reference's goldens, the _many drop-ins against loops of the single searches, the
batch path after bow(), and concurrent callers."""
import ctypes as C
import threading

import numpy as np
import pytest

import bow_match_cases as BC
import bow_match_oracle as O
import matcher_world as MW
import vocab_synth as VS
from test_bow_match_cpu import golden_scenes

pytestmark = pytest.mark.gpu

CASES = BC.all_cases()
ORACLE = {c["name"]: BC.oracle(c) for c in CASES}  # computed once, shared, never modified
RAW = ("match12", "match21", "bin12", "hist", "n_raw")


def run_host(case):
    from pyorbslam_amd.matcher import bow_match_arrays
    a = BC.pack(case["frames"])
    return bow_match_arrays(a["desc"], a["angle"], a["off"], a["fv_off"], a["fv_node"], a["fv_end"], a["fv_idx"],
                            np.array(case["pairs"], np.int32).reshape(-1, 2), case["th"], case["inclusive"],
                            case["nnratio"], a["elig"] if case["use_elig1"] else None,
                            a["elig"] if case["use_elig2"] else None)


def assert_raw(case, got, want, where=""):
    assert got["status"] == 0
    for p, ((a, b), w) in enumerate(zip(case["pairs"], want)):
        n1, n2 = len(case["frames"][a]["desc"]), len(case["frames"][b]["desc"])
        tag = f"{case['name']}{where} pair {p}"
        assert np.array_equal(got["match12"][p, :n1], w[0]), tag
        assert np.array_equal(got["match21"][p, :n2], w[1]), tag
        assert np.array_equal(got["bin12"][p, :n1], w[2]), tag
        assert np.array_equal(got["hist"][p], w[3]), tag
        assert int(got["n_raw"][p]) == w[4], tag
        assert bool((got["match12"][p, n1:] == -1).all()) and bool((got["match21"][p, n2:] == -1).all()), tag


# ---- 1. host entry: every case, all five raw outputs, bit for bit --------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_entry_matches_the_oracle(case):
    from pyorbslam_amd.matcher import ORBMatcher
    got = run_host(case)
    want = ORACLE[case["name"]]
    assert_raw(case, got, want)
    m = ORBMatcher(case["nnratio"], True)
    for p, ((a, b), w) in enumerate(zip(case["pairs"], want)):
        n1, n2 = len(case["frames"][a]["desc"]), len(case["frames"][b]["desc"])
        r = m._bow_reject(got["match12"][p, :n1], got["match21"][p, :n2], got["bin12"][p, :n1], got["hist"][p],
                          int(got["n_raw"][p]))
        if case["stable_cut"]:
            e = O.reject(*w)
        else:  # the cut is a tie: only this process's own compute_three_maxima says which bins stay
            e = O.reject(*w, keep=m.compute_three_maxima([range(c) for c in w[3][:30].tolist()], 30))
        assert np.array_equal(r[0], e[0]) and np.array_equal(r[1], e[1]) and r[2] == e[2]


def test_no_pairs_launch_nothing():
    from pyorbslam_amd import _lib
    case = CASES[0]
    c0 = dict(case, pairs=[])
    got = run_host(c0)
    assert got["match12"].shape[0] == 0 and got["n_raw"].shape == (0,) and got["status"] == 0
    ms = C.c_float(-1)
    assert _lib.lib().orbfe_bow_match_last_ms(C.byref(ms)) == 0 and ms.value >= 0


# ---- 2. device entry --------------------------------------------------------------------------------------------------
GUARD = -9


class Device:
    """Strided frames on the device as orbfe_bow_match_device takes them: keypoint records for the angles, counts
    at a stride of two with poison between, and guard rows around (and guard entries behind) every output."""

    def __init__(self, frames, frame_stride, fv_stride, out_stride, n_pairs, counts=None):
        import torch
        from pyorbslam_amd import _lib
        F = len(frames)
        self.torch, self.F, self.fs, self.fvs, self.os, self.P = torch, F, frame_stride, fv_stride, out_stride, n_pairs
        desc = np.full((F, frame_stride, 32), 0xFF, np.uint8)
        kps = np.full((F, frame_stride, 6), np.nan, np.float32)
        elig = np.zeros((F, frame_stride + 3), np.uint8)  # its own stride
        node = np.full((F, fv_stride), 12345, np.int32)
        end = np.full((F, fv_stride), 12345, np.int32)
        idx = np.full((F, fv_stride), 12345, np.int32)
        nn = np.zeros(F, np.int32)
        cnt = np.full(2 * F, 54321, np.int32)
        for f, fr in enumerate(frames):
            n = len(fr["desc"])
            desc[f, :n], kps[f, :n, 3], elig[f, :n] = fr["desc"], fr["angle"], fr["elig"]
            k = len(fr["fv_node"])
            node[f, :k], end[f, :k], idx[f, :len(fr["fv_idx"])], nn[f] = fr["fv_node"], fr["fv_end"], fr["fv_idx"], k
            cnt[2 * f] = n if counts is None else counts[f]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.d = dict(desc=up(desc), kps=up(kps), elig=up(elig), node=up(node), end=up(end), idx=up(idx), nn=up(nn),
                      cnt=up(cnt))
        self.fv = _lib.BowOut(n_nodes=self.d["nn"].data_ptr(), fv_node=self.d["node"].data_ptr(),
                              fv_end=self.d["end"].data_ptr(), fv_idx=self.d["idx"].data_ptr())
        P = n_pairs
        self.m = torch.full((2, P + 2, out_stride), GUARD, dtype=torch.int32, device="cuda")
        self.b = torch.full((P + 2, out_stride), GUARD, dtype=torch.int8, device="cuda")
        self.hist = torch.full((P + 2, 32), GUARD, dtype=torch.int32, device="cuda")
        self.n_raw = torch.full((P + 2,), GUARD, dtype=torch.int32, device="cuda")
        self.status = torch.zeros(3, dtype=torch.int32, device="cuda")
        self.out = _lib.BowMatchOut(match12=self.m[0, 1].data_ptr(), match21=self.m[1, 1].data_ptr(),
                                    bin12=self.b[1].data_ptr(), hist=self.hist[1].data_ptr(),
                                    n_raw=self.n_raw[1:].data_ptr(), status=self.status[1:].data_ptr())

    def run(self, pairs, th=50, inclusive=False, nnratio=1.0, use_elig1=True, use_elig2=True):
        from pyorbslam_amd import _lib
        torch = self.torch
        d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda").reshape(-1, 2)
        s = torch.cuda.current_stream()
        e = self.d["elig"].data_ptr()
        rc = _lib.lib().orbfe_bow_match_device(
            self.d["desc"].data_ptr(), self.fs, self.d["cnt"].data_ptr(), 2, self.F,
            self.d["kps"].data_ptr() + 12, 6, e if use_elig1 else None, self.fs + 3, e if use_elig2 else None,
            self.fs + 3, C.byref(self.fv), self.fvs, d_pairs.data_ptr(), len(pairs), th, int(inclusive), nnratio,
            C.byref(self.out), self.os, C.c_void_p(s.cuda_stream))
        s.synchronize()
        return rc

    def result(self):
        m, b = self.m.cpu().numpy(), self.b.cpu().numpy()
        return dict(match12=m[0, 1:-1], match21=m[1, 1:-1], bin12=b[1:-1], hist=self.hist.cpu().numpy()[1:-1],
                    n_raw=self.n_raw.cpu().numpy()[1:-1], status=int(self.status[1]))

    def guards_intact(self):
        m, b = self.m.cpu().numpy(), self.b.cpu().numpy()
        st = self.status.cpu().numpy()
        return (bool((m[:, [0, -1]] == GUARD).all()) and bool((b[[0, -1]] == GUARD).all())
                and bool((self.hist.cpu().numpy()[[0, -1]] == GUARD).all())
                and bool((self.n_raw.cpu().numpy()[[0, -1]] == GUARD).all()) and st[0] == 0 and st[2] == 0)

    def assert_pair(self, p, want, n1, n2, tag):
        r = self.result()
        assert np.array_equal(r["match12"][p, :n1], want[0][:n1]), tag
        assert np.array_equal(r["match21"][p, :n2], want[1][:n2]), tag
        assert np.array_equal(r["bin12"][p, :n1], want[2][:n1]), tag
        assert np.array_equal(r["hist"][p], want[3]) and int(r["n_raw"][p]) == want[4], tag
        # nothing behind the frames' lengths
        assert bool((r["match12"][p, n1:] == GUARD).all()) and bool((r["match21"][p, n2:] == GUARD).all()), tag
        assert bool((r["bin12"][p, n1:] == GUARD).all()), tag


def truncated(f, n):
    """Frame f cut to its first n features: what a clamped count leaves (indices past n drop out of the runs)."""
    node, end, idx, a = [], [], [], 0
    for k, e in zip(f["fv_node"].tolist(), f["fv_end"].tolist()):
        idx += [i for i in f["fv_idx"][a:e].tolist() if i < n]
        node.append(k)
        end.append(len(idx))
        a = e
    return dict(desc=f["desc"][:n], angle=f["angle"][:n], elig=f["elig"][:n], fv_node=np.array(node, np.int32),
                fv_end=np.array(end, np.int32), fv_idx=np.array(idx, np.int32))


def test_device_entry_strides_guards_and_record_angles():
    """The sharing case's nine pairs through the device entry: keypoint-record angle stride, an eligibility stride of
    its own, poisoned counts between the real ones, guards around every output."""
    case = next(c for c in CASES if c["name"] == "sharing_waves_plus_one_pairs")
    frames = [dict(f, angle=(f["angle"] + np.float32(37.5 * k)).astype(np.float32)) for k, f in enumerate(case["frames"])]
    dev = Device(frames, frame_stride=40, fv_stride=33, out_stride=35, n_pairs=len(case["pairs"]))
    assert dev.run(case["pairs"], nnratio=0.9) == 0
    assert dev.guards_intact() and dev.result()["status"] == 0
    bins = set()
    for p, (a, b) in enumerate(case["pairs"]):
        want = O.match_pair(frames[a], frames[b], True, True, 50, False, 0.9)
        dev.assert_pair(p, want, 30, 30, f"pair {p}")
        bins |= set(np.flatnonzero(want[3]).tolist())
    assert len(bins) > 2  # the angles were read from the records, at their stride
    # the kf_f form: inclusive threshold, no eligibility on side 2
    dev2 = Device(frames, 40, 33, 35, 2)
    assert dev2.run([(0, 1), (2, 2)], inclusive=True, nnratio=0.8, use_elig2=False) == 0
    for p, (a, b) in enumerate([(0, 1), (2, 2)]):
        dev2.assert_pair(p, O.match_pair(frames[a], frames[b], True, False, 50, True, 0.8), 30, 30, f"kf_f pair {p}")
    assert dev2.guards_intact()


def test_device_entry_clamps_counts_and_flags_bad_pairs():
    from pyorbslam_amd import _lib
    frames = BC.sharing_frames()
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0)]
    # counts above out_stride (frame 1) and below zero (frame 3)
    dev = Device(frames, 40, 33, 25, 4, counts=[20, 30, 25, -4])
    assert dev.run(pairs, nnratio=0.9) == 0
    assert dev.result()["status"] == _lib.ORBFE_BOW_OVER_OUT | _lib.ORBFE_BOW_NEGATIVE and dev.guards_intact()
    cut = [truncated(f, n) for f, n in zip(frames, [20, 25, 25, 0])]
    for p, (a, b) in enumerate(pairs):
        dev.assert_pair(p, O.match_pair(cut[a], cut[b], True, True, 50, False, 0.9), len(cut[a]["desc"]),
                        len(cut[b]["desc"]), f"clamped pair {p}")
    # a count above the frame stride
    dev = Device(frames, 30, 33, 64, 1, counts=[31, 30, 30, 30])
    assert dev.run([(0, 1)], nnratio=0.9) == 0
    assert dev.result()["status"] == _lib.ORBFE_BOW_OVER_FRAME and dev.guards_intact()
    dev.assert_pair(0, O.match_pair(frames[0], frames[1], True, True, 50, False, 0.9), 30, 30, "over frame")
    # pairs that name frames that do not exist: flagged, unmatched, the existing side filled with -1
    dev = Device(frames, 40, 33, 35, 3)
    assert dev.run([(0, 4), (-1, 2), (1, 1)], nnratio=0.9) == 0
    r = dev.result()
    assert r["status"] == _lib.ORBFE_BOW_BAD_PAIR and dev.guards_intact()
    assert r["n_raw"].tolist()[:2] == [0, 0] and not r["hist"][:2].any()
    assert bool((r["match12"][0, :30] == -1).all()) and bool((r["match12"][0, 30:] == GUARD).all())
    assert bool((r["match21"][0] == GUARD).all()) and bool((r["match12"][1] == GUARD).all())
    assert bool((r["match21"][1, :30] == -1).all())
    dev.assert_pair(2, O.match_pair(frames[1], frames[1], True, True, 50, False, 0.9), 30, 30, "the good pair")


def test_device_entry_frame_above_the_cap():
    """A count above ORBFE_BOW_MAX_FRAME is clamped to it and flagged; the feature past the cap stays unmatched."""
    import torch  # noqa: F401
    from pyorbslam_amd import _lib
    cap = _lib.ORBFE_BOW_MAX_FRAME
    n = cap + 4
    f = dict(desc=np.tile(BC.D(), (n, 1)), angle=np.zeros(n, np.float32), elig=np.ones(n, np.uint8),
             fv_node=np.array([3], np.int32), fv_end=np.array([3], np.int32), fv_idx=np.array([cap + 1, 5, cap - 1], np.int32))
    g = dict(f, desc=f["desc"].copy(), fv_idx=np.array([cap - 1, cap + 2, 7], np.int32))
    g["desc"][cap - 1], g["desc"][7] = BC.D(0), BC.D(0, 1)  # distances 1 and 2 from every feature of f
    dev = Device([f, g], n, 8, n, 1)
    assert dev.run([(0, 1)], nnratio=1.5) == 0
    r = dev.result()
    assert r["status"] == _lib.ORBFE_BOW_OVER_MAX and dev.guards_intact()
    want = O.match_pair(truncated(f, cap), truncated(g, cap), True, True, 50, False, 1.5)
    dev.assert_pair(0, want, cap, cap, "above the cap")
    assert want[4] == 2 and want[0][5] == cap - 1 and want[0][cap - 1] == 7


# ---- 3. the reference's goldens ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kf_kf", "kf_f"])
def test_goldens_through_the_host_entry(kind):
    from pyorbslam_amd.matcher import ORBMatcher, bow_match_arrays
    scenes = golden_scenes(kind)
    a = BC.pack([f for f1, f2, _ in scenes for f in (f1, f2)])
    pairs = np.array([[2 * s, 2 * s + 1] for s in range(len(scenes))], np.int32)
    for c in range(4):
        nn, ori = scenes[0][2][c][:2]
        got = bow_match_arrays(a["desc"], a["angle"], a["off"], a["fv_off"], a["fv_node"], a["fv_end"], a["fv_idx"],
                               pairs, 50, kind == "kf_f", nn, a["elig"], a["elig"] if kind == "kf_kf" else None)
        assert got["status"] == 0
        for s, (f1, f2, runs) in enumerate(scenes):
            n1, n2 = len(f1["desc"]), len(f2["desc"])
            r = ORBMatcher(nn, ori)._bow_reject(got["match12"][s, :n1], got["match21"][s, :n2], got["bin12"][s, :n1],
                                                got["hist"][s], int(got["n_raw"][s]))
            assert r[2] == runs[c][2], (kind, s, c)
            assert np.array_equal(r[0] if kind == "kf_kf" else r[1], runs[c][3]), (kind, s, c)


# ---- 4. the _many drop-ins ----------------------------------------------------------------------------------------------
class _Z:
    def __init__(self, d):
        self._d, self.files = d, list(d.keys())

    def __getitem__(self, k):
        return self._d[k]


@pytest.fixture(scope="module")
def world_arrays():
    rng = np.random.Generator(np.random.PCG64(9400))
    return _Z(MW.make_world(rng, n_kf=9, n=300, n_mp=220, with_frame=True, n_words=40))


def same_results(got, want):
    assert len(got) == len(want)
    for (gn, gl), (wn, wl) in zip(got, want):
        assert gn == wn and len(gl) == len(wl)
        assert all(a is b for a, b in zip(gl, wl))  # the same map-point objects, or None


@pytest.mark.parametrize("n_cand", [1, 3, 8])
@pytest.mark.parametrize("nn,ori", [(1, True), (0.7, True), (0.8, False)])
def test_many_equal_a_loop_of_single_searches(world_arrays, n_cand, nn, ori):
    from pyorbslam_amd.matcher import ORBMatcher
    w = MW.build(world_arrays)
    m = ORBMatcher(nn, ori)
    want = [m.search_by_BoW_kf_kf(w.kfs[0], kf) for kf in w.kfs[1:1 + n_cand]]
    got = m.search_by_BoW_kf_kf_many(w.kfs[0], w.kfs[1:1 + n_cand])
    same_results(got, want)
    assert sum(n for n, _ in got) > 10 * n_cand
    cands = [w.kfs[0]] + w.kfs[1:n_cand]
    want = [m.search_by_BoW_kf_f(kf, w.frame) for kf in cands]
    got = m.search_by_BoW_kf_f_many(cands, w.frame)
    same_results(got, want)
    assert got[0][0] > 10


def test_many_fall_back_per_element(world_arrays, monkeypatch):
    """A float32 angle in one candidate: that element takes the single search, the others the launch."""
    from pyorbslam_amd import matcher
    w = MW.build(world_arrays)
    m = matcher.ORBMatcher(0.9, True)
    w.kfs[2].mvKeysUn[5].angle = np.float32(w.kfs[2].mvKeysUn[5].angle)
    want = [m.search_by_BoW_kf_kf(w.kfs[0], kf) for kf in w.kfs[1:4]]
    want_f = [m.search_by_BoW_kf_f(kf, w.frame) for kf in w.kfs[1:4]]
    singles, launches = [], []
    kk, kf_f, arrays = m.search_by_BoW_kf_kf, m.search_by_BoW_kf_f, matcher.bow_match_arrays
    monkeypatch.setattr(m, "search_by_BoW_kf_kf", lambda a, b: singles.append(b) or kk(a, b))
    monkeypatch.setattr(m, "search_by_BoW_kf_f", lambda a, b: singles.append(a) or kf_f(a, b))
    monkeypatch.setattr(matcher, "bow_match_arrays", lambda *a, **k: launches.append(len(a[7])) or arrays(*a, **k))
    same_results(m.search_by_BoW_kf_kf_many(w.kfs[0], w.kfs[1:4]), want)
    same_results(m.search_by_BoW_kf_f_many(w.kfs[1:4], w.frame), want_f)
    assert singles == [w.kfs[2], w.kfs[2]] and launches == [2, 2]


# ---- 5. the batch path ---------------------------------------------------------------------------------------------------
def test_batch_match_bow_after_bow():
    import torch
    from pyorbslam_amd import synth
    from pyorbslam_amd.batch import StereoFrontEnd
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    tree = VS.make_tree(seed=81, k=6, L=3, p_stop=0.2, p_dup=0.1, p_zero=0.1)
    v = TemplatedVocabulary(k=tree["k"], L=tree["L"]).from_arrays(tree["parent"], tree["is_leaf"], tree["desc"],
                                                                  tree["weight"])
    imgs = torch.from_numpy(np.stack([im for s in (3, 4, 5, 6) for im in synth.make_pair(s, 211, 157)])).cuda()
    fe = StereoFrontEnd(211, 157, max_pairs=4, nfeatures=500)
    s = torch.cuda.current_stream()
    with pytest.raises(RuntimeError):
        fe.match_bow([(0, 1)])
    fe.enqueue(imgs, stream_ptr=s.cuda_stream)
    assert fe.bow(v, levels_up=2, side="left", stream_ptr=s.cuda_stream) == 4
    pairs = [(0, 1), (1, 2), (2, 2), (3, 0)]
    frames = []
    for p in range(4):
        kps, desc = fe.fetch_image(2 * p)
        a = fe.fetch_bow(p)
        st = fe.fetch_stereo(p)["status"]
        frames.append(dict(desc=desc, angle=kps["angle"].astype(np.float32), elig=(st != 0).astype(np.uint8),
                           fv_node=a.node, fv_end=a.end, fv_idx=a.idx))
    assert all(len(f["desc"]) > 50 and 0 < int(f["elig"].sum()) < len(f["desc"]) for f in frames)
    total = 0
    for eligible, use in ((None, False), ("stereo", True)):
        assert fe.match_bow(pairs, th=50, inclusive=False, nnratio=0.9, eligible=eligible, stream_ptr=s.cuda_stream) == 4
        for p, (a, b) in enumerate(pairs):
            raw = O.match_pair(frames[a], frames[b], use, use, 50, False, 0.9)
            got = fe.fetch_bow_matches(p, check_orientation=False)
            assert np.array_equal(got[0], raw[0]) and np.array_equal(got[1], raw[1]) and got[2] == raw[4], (eligible, p)
            if O.cut_is_stable(raw[3]):
                got = fe.fetch_bow_matches(p)
                e = O.reject(*raw)
                assert np.array_equal(got[0], e[0]) and np.array_equal(got[1], e[1]) and got[2] == e[2], (eligible, p)
            total += raw[4]
    assert total > 40 and fe.bow_status() == 0
    mask = np.zeros((4, fe.kp_cap), np.uint8)
    for p, f in enumerate(frames):
        mask[p, :len(f["desc"]):2] = 1
    fe.match_bow([(1, 3)], inclusive=True, nnratio=0.8, eligible=mask, stream_ptr=s.cuda_stream)
    ev = [dict(f, elig=mask[p, :len(f["desc"])]) for p, f in enumerate(frames)]
    raw = O.match_pair(ev[1], ev[3], True, True, 50, True, 0.8)
    got = fe.fetch_bow_matches(0, check_orientation=False)
    assert np.array_equal(got[0], raw[0]) and got[2] == raw[4]
    with pytest.raises(IndexError):
        fe.fetch_bow_matches(1)
    assert fe.bow(v, levels_up=2, side="both", stream_ptr=s.cuda_stream) == 8
    with pytest.raises(ValueError):
        fe.match_bow(pairs, eligible="stereo", stream_ptr=s.cuda_stream)
    fe.match_bow([(0, 9)], stream_ptr=s.cuda_stream)
    from pyorbslam_amd import _lib
    assert fe.bow_status() == _lib.ORBFE_BOW_BAD_PAIR


# ---- 6. four threads ---------------------------------------------------------------------------------------------------
def test_four_threads_get_their_own_results():
    names = ["run2_129", "blocking_3_nn0.6", "sharing_waves_plus_one_pairs", "nodes_many"]
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
