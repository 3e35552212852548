"""k_bow_assemble on the GPU: BoW and feature vectors of whole frames assembled on the device, bit for bit against
the reference's own outputs (tests/golden/vocab_*.npz) and VocabOracle.transform (an explicit sequential sum, never
sum()).  The inputs come from tests/bow_assemble_cases.py; tests/test_bow_assemble_cases_cpu.py shows that they
reach what they aim at.

Sizes named for the implementation: a frame of up to 2 048 features takes a 256-thread workgroup, a longer one a
1 024-thread workgroup (AC.WORKGROUPS); the bitonic sort pads the kept features to 2, 4, .., 8 192 (AC.PADDED).
AC.EDGE_LENGTHS holds each of them and its neighbours."""
import ctypes as C
import threading

import numpy as np
import pytest

import bow_assemble_cases as AC
import vocab_synth as VS
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def native_of(t):
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    return TemplatedVocabulary(k=t["k"], L=t["L"]).from_arrays(t["parent"], t["is_leaf"], t["desc"], t["weight"])


# ---- 1. the reference's own outputs ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k5L3", "k10L4_ragged", "k20L2_ties", "wide"])
def test_bow_many_reference_golden(case):
    z = np.load(GOLDEN / f"vocab_{case}.npz", allow_pickle=False)
    t = dict(k=int(z["k"]), L=int(z["L"]), parent=z["parent"], is_leaf=z["is_leaf"], desc=z["desc"],
             weight=z["weight"])
    q = z["queries"] if "queries" in z.files else np.ascontiguousarray(z["desc"][z["query_node"]])
    v = native_of(t)
    if case == "wide":
        assert len(q) == 4664
    for lu in z["levels_up"].tolist():
        a, empty = v.bow_many([q, q[:0]], lu)
        assert a.word.dtype == np.int32 and np.array_equal(a.word, z[f"bv_word_{lu}"])
        assert np.array_equal(a.weight.view(np.uint64), z[f"bv_w_{lu}"].view(np.uint64))
        assert np.array_equal(a.node, z[f"fv_node_{lu}"])
        assert np.array_equal(np.diff(a.end, prepend=0), z[f"fv_len_{lu}"])
        assert np.array_equal(a.idx, z[f"fv_idx_{lu}"]) and a.n_kept == len(z[f"fv_idx_{lu}"])
        assert empty.n_kept == 0 and len(empty.word) == 0 and len(empty.node) == 0


# ---- 2. every frame length in one launch ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["small", "wide"])
def test_frame_lengths_in_one_launch(which):
    tree, seed, pool = (AC.small_tree(), 41, 600) if which == "small" else (AC.wide_tree(), 43, 6000)
    frames = AC.length_frames(tree, seed, pool)
    o = AC.PoolOracle(tree)
    v = native_of(tree)
    got = v.bow_many(frames, AC.LEVELS_UP)
    assert len(got) == len(frames)
    for f, a in zip(frames, got):
        AC.assert_arrays(a, o.transform(f, AC.LEVELS_UP), f"{which} tree, {len(f)} features")
    assert v.last_bow_ms() > 0
    # the dict surface over the same launch shape: same keys in the same order, Python floats and ints
    short = [f for f in frames if len(f) <= 300]
    for f, (bv, fv) in zip(short, v.transform_many(short, AC.LEVELS_UP)):
        want = o.transform(f, AC.LEVELS_UP)
        assert list(bv.items()) == list(want[0].items()) and list(fv.items()) == list(want[1].items())
        assert all(type(x) is float for x in bv.values()) and all(type(k) is int for k in list(bv) + list(fv))
        assert (bv, fv) == ({}, {}) or (type(bv).__name__, type(fv).__name__) == ("OrderedDict", "OrderedDict")


# ---- 3. the limit --------------------------------------------------------------------------------------------------
def test_frame_above_the_limit():
    from pyorbslam_amd._lib import ORBFE_BOW_MAX_FRAME, ORBFE_EINVAL, OrbfeError
    tree = AC.small_tree()
    o = AC.PoolOracle(tree)
    v = native_of(tree)
    pool = VS.query_descriptors(tree, 61, 500)
    f = pool[np.random.default_rng(62).integers(0, len(pool), ORBFE_BOW_MAX_FRAME + 1)]
    with pytest.raises(OrbfeError) as e:
        v.bow_many([pool[:10], f], AC.LEVELS_UP)
    assert e.value.code == ORBFE_EINVAL and f"limit of {ORBFE_BOW_MAX_FRAME} per frame" in str(e.value)
    want = o.transform(f, AC.LEVELS_UP)
    for got in (v.transform(f, AC.LEVELS_UP), v.transform_many([pool[:10], f, f[:-1]], AC.LEVELS_UP)[1]):
        assert list(got[0].items()) == list(want[0].items()) and list(got[1].items()) == list(want[1].items())
    AC.assert_arrays(v.bow_many([f[:-1]], AC.LEVELS_UP)[0], o.transform(f[:-1], AC.LEVELS_UP), "the longest frame")


# ---- 4. threading across frames, long runs, dropped, negative and all-dropped frames -------------------------------
def test_special_frames():
    tree = AC.small_tree()
    o = AC.PoolOracle(tree)
    fr = AC.special_frames(tree, o, 51)
    v = native_of(tree)
    got = v.bow_many(list(fr.values()), AC.LEVELS_UP)
    for (name, f), a in zip(fr.items(), got):
        AC.assert_arrays(a, o.transform(f, AC.LEVELS_UP), name)
    assert got[list(fr).index("all_dropped")].n_kept == 0
    assert v.transform(fr["all_dropped"], AC.LEVELS_UP) == ({}, {})
    assert len(got[list(fr).index("one_word")].word) == 1


def test_negative_and_nan_weights_drop_the_feature():
    t, _, _ = AC.patched_tree()
    o = AC.PoolOracle(t)
    v = native_of(t)
    pool = VS.query_descriptors(t, 33, 400)
    frames = [pool, pool[::-1].copy(), pool[100:103]]
    for f, a in zip(frames, v.bow_many(frames, AC.LEVELS_UP)):
        AC.assert_arrays(a, o.transform(f, AC.LEVELS_UP), "patched weights")


# ---- 5. the device entry ---------------------------------------------------------------------------------------------
class DeviceOut:
    """Output arrays for n frames of `stride` entries, each with `guard` sentinel entries on both sides."""
    SENT = -77

    def __init__(self, n, stride, guard=64):
        import torch
        from pyorbslam_amd._lib import BowOut
        self.n, self.stride, self.guard = n, stride, guard
        mk = lambda m, dt: torch.full((m + 2 * guard,), self.SENT, dtype=dt, device="cuda")  # noqa: E731
        self.t = {k: mk(n * stride, torch.int32) for k in ("bow_word", "fv_node", "fv_end", "fv_idx")}
        self.t["bow_weight"] = mk(n * stride, torch.float64)
        self.t.update({k: mk(n, torch.int32) for k in ("n_words", "n_nodes", "n_kept")})
        self.t["status"] = mk(1, torch.int32)
        self.t["status"][guard] = 0
        self.out = BowOut(**{k: x.data_ptr() + guard * x.element_size() for k, x in self.t.items()})

    def host(self, k):
        return self.t[k].cpu().numpy()

    def guards_intact(self):
        return all(bool((h[:self.guard] == self.SENT).all()) and bool((h[-self.guard:] == self.SENT).all())
                   for h in (self.host(k) for k in self.t))

    def untouched(self):
        return all(bool((np.delete(self.host(k), self.guard if k == "status" else []) == self.SENT).all())
                   for k in self.t)

    def frame(self, f):
        from pyorbslam_amd.vocabulary import BowArrays
        g, s = self.guard, self.stride
        nw, nn, nk = (int(self.host(k)[g + f]) for k in ("n_words", "n_nodes", "n_kept"))
        cut = lambda k, m: self.host(k)[g + f * s:g + f * s + m].copy()  # noqa: E731
        return BowArrays(cut("bow_word", nw), cut("bow_weight", nw), cut("fv_node", nn), cut("fv_end", nn),
                         cut("fv_idx", nk), nk)

    def status(self):
        return int(self.host("status")[self.guard])


def run_device(v, desc, frame_stride, count, count_stride, n_frames, out_stride, out, offset=0, scratch_slack=0):
    import torch
    from pyorbslam_amd._lib import lib
    need = C.c_int64()
    assert lib().orbfe_vocab_bow_scratch_bytes(n_frames, frame_stride, C.byref(need)) == 0
    scratch = torch.zeros(need.value // 8 + 1 + scratch_slack, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    rc = lib().orbfe_vocab_bow_device(v._handle(), C.c_void_p(desc.data_ptr() + offset), frame_stride,
                                      C.c_void_p(count.data_ptr()), count_stride, n_frames, v.L - AC.LEVELS_UP,
                                      out_stride, C.byref(out.out), C.c_void_p(scratch.data_ptr()), need.value,
                                      C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc


def test_device_entry_strided_frames():
    """Frames at a stride with counts on the device (0, 1, the stride itself), count_stride 2 with poisoned counts
    between, and 0xFF descriptors behind every count."""
    import torch
    tree = AC.small_tree()
    o = AC.PoolOracle(tree)
    v = native_of(tree)
    stride = 300
    counts = [0, 300, 1, 257, 0, 64, 299]
    pool = VS.query_descriptors(tree, 71, 500)
    rng = np.random.default_rng(72)
    frames = [pool[rng.integers(0, len(pool), n)] for n in counts]
    desc = np.full((len(counts), stride, 32), 0xFF, np.uint8)
    for f, q in enumerate(frames):
        desc[f, :len(q)] = q
    cnt = np.full(2 * len(counts), 12345, np.int32)     # the odd entries are never read
    cnt[::2] = counts
    d_desc, d_cnt = torch.from_numpy(desc).cuda(), torch.from_numpy(cnt).cuda()
    out = DeviceOut(len(counts), stride)
    assert run_device(v, d_desc, stride, d_cnt, 2, len(counts), stride, out) == 0
    assert out.status() == 0 and out.guards_intact()
    for f, q in enumerate(frames):
        AC.assert_arrays(out.frame(f), o.transform(q, AC.LEVELS_UP), f"frame {f}, {len(q)} descriptors")
    # the poison is what a count protects from: frame 2 with it counted in gives something else
    assert o.transform(desc[2][:5], AC.LEVELS_UP) != o.transform(frames[2], AC.LEVELS_UP)


def test_device_entry_refusals_and_empty_launch():
    import torch
    from pyorbslam_amd._lib import ORBFE_EINVAL, lib
    tree = AC.small_tree()
    v = native_of(tree)
    d_desc = torch.zeros(4 * 64 * 32 + 64, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((4,), 64, dtype=torch.int32, device="cuda")
    out = DeviceOut(4, 64)
    assert d_desc.data_ptr() % 16 == 0
    assert run_device(v, d_desc, 64, d_cnt, 1, 4, 64, out, offset=8) == ORBFE_EINVAL
    assert b"aligned" in lib().orbfe_last_error() and out.untouched()
    assert run_device(v, d_desc, 64, d_cnt, 1, 0, 64, out) == 0
    assert out.untouched()
    assert run_device(v, d_desc, 64, d_cnt, 1, 4, 64, out, offset=16) == 0
    assert not out.untouched() and out.guards_intact() and out.status() == 0


def test_device_entry_clamps_counts():
    """Counts above out_stride, above the frame stride, above ORBFE_BOW_MAX_FRAME and below zero: flagged, clamped,
    nothing outside the frame's block."""
    import torch
    from pyorbslam_amd import _lib
    tree = AC.small_tree()
    o = AC.PoolOracle(tree)
    v = native_of(tree)
    stride, out_stride = 96, 40
    pool = VS.query_descriptors(tree, 73, 500)
    desc = pool[np.random.default_rng(74).integers(0, len(pool), 4 * stride)].reshape(4, stride, 32)
    d_desc = torch.from_numpy(np.ascontiguousarray(desc)).cuda()

    def run(counts, out_stride):
        out = DeviceOut(4, out_stride)
        d_cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
        assert run_device(v, d_desc, stride, d_cnt, 1, 4, out_stride, out) == 0
        assert out.guards_intact()
        return out

    out = run([10, 41, 40, 0], out_stride)
    assert out.status() == _lib.ORBFE_BOW_OVER_OUT
    for f, n in enumerate([10, 40, 40, 0]):
        AC.assert_arrays(out.frame(f), o.transform(desc[f][:n], AC.LEVELS_UP), f"frame {f} clamped to {n}")
    out = run([96, 97, 1 << 20, -3], 128)
    assert out.status() == _lib.ORBFE_BOW_OVER_FRAME | _lib.ORBFE_BOW_OVER_OUT | _lib.ORBFE_BOW_NEGATIVE
    for f, n in enumerate([96, 96, 96, 0]):
        AC.assert_arrays(out.frame(f), o.transform(desc[f][:n], AC.LEVELS_UP), f"frame {f} clamped to {n}")
    big = DeviceOut(1, 9000)
    d_big = torch.zeros((9000, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.tensor([8500], dtype=torch.int32, device="cuda")
    assert run_device(v, d_big, 9000, d_cnt, 1, 1, 9000, big) == 0
    assert big.status() == _lib.ORBFE_BOW_OVER_MAX and big.guards_intact()
    AC.assert_arrays(big.frame(0), o.transform(np.zeros((8192, 32), np.uint8), AC.LEVELS_UP), "clamped to the limit")


# ---- 6. batch end to end ---------------------------------------------------------------------------------------------
def test_batch_to_bow_to_database():
    import torch
    from pyorbslam_amd import synth
    from pyorbslam_amd.batch import StereoFrontEnd
    from pyorbslam_amd.kfdb import BowDatabase
    tree = VS.make_tree(seed=81, k=6, L=3, p_stop=0.2, p_dup=0.1, p_zero=0.1)
    v = native_of(tree)
    pairs = [synth.make_pair(s, 211, 157) for s in (3, 4)]
    imgs = torch.from_numpy(np.stack([im for p in pairs for im in p])).cuda()
    fe = StereoFrontEnd(211, 157, max_pairs=2, nfeatures=500)
    s = torch.cuda.current_stream()
    fe.enqueue(imgs, stream_ptr=s.cuda_stream)
    desc = [fe.fetch_image(i)[1] for i in range(4)]
    assert all(len(d) > 50 for d in desc)
    want = [v.transform(d, 1) for d in desc]
    for side, images in (("both", [0, 1, 2, 3]), ("left", [0, 2])):
        assert fe.bow(v, levels_up=1, side=side, stream_ptr=s.cuda_stream) == len(images)
        for f, i in enumerate(images):
            a = fe.fetch_bow(f)
            got = a.dicts()
            assert list(got[0].items()) == list(want[i][0].items()), (side, i)
            assert list(got[1].items()) == list(want[i][1].items()), (side, i)
        assert fe.bow_status() == 0
        with pytest.raises(IndexError):
            fe.fetch_bow(len(images))
    # the fetched arrays are what the database takes
    fe.bow(v, levels_up=1, side="both", stream_ptr=s.cuda_stream)
    arrs = [fe.fetch_bow(i) for i in range(4)]
    db_a, db_d = BowDatabase(8, 4096), BowDatabase(8, 4096)
    for a, w in zip(arrs, want):
        assert db_a.add_arrays(a.word, a.weight) == db_d.add(w[0])
    for a, w in zip(arrs, want):
        ra, rd = db_a.query_arrays(a.word, a.weight), db_d.query(w[0])
        assert np.array_equal(ra[0], rd[0]) and np.array_equal(ra[1], rd[1])
        assert np.array_equal(np.asarray(ra[2]).view(np.uint64), np.asarray(rd[2]).view(np.uint64))


# ---- 7. one vocabulary under four threads ----------------------------------------------------------------------------
def test_bow_many_and_transform_shared_by_threads():
    tree = AC.small_tree()
    o = AC.PoolOracle(tree)
    v = native_of(tree)
    pool = VS.query_descriptors(tree, 91, 600)
    rng = np.random.default_rng(92)
    frames = [pool[rng.integers(0, len(pool), int(n))] for n in rng.integers(0, 700, 24)]
    want = [o.transform(f, AC.LEVELS_UP) for f in frames]
    single = v.bow_many(frames, AC.LEVELS_UP)
    errors = []

    def work(k):
        try:
            for it in range(6):
                mine = list(range((k + it) % 4, len(frames), 4))
                got = v.bow_many([frames[i] for i in mine], AC.LEVELS_UP)
                for i, a in zip(mine, got):
                    for x, y in zip(a[:5], single[i][:5]):
                        if not np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)):
                            errors.append(("bow_many", k, it, i))
                    AC.assert_arrays(a, want[i], f"thread {k}")
                i = mine[it % len(mine)]
                t = v.transform(frames[i], AC.LEVELS_UP)
                if list(t[0].items()) != list(want[i][0].items()) or list(t[1].items()) != list(want[i][1].items()):
                    errors.append(("transform", k, it, i))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(("raised", k, repr(e)))

    ths = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors[:5]
