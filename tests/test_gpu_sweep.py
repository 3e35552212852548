"""Every batch launch shape at small geometries and mixed content, every image and pair against the oracle.

The geometry sweep walks the level-0 sizes on which the kernels' tails depend (w mod 30 and h mod 30: the
narrower last FAST cell column / row and levels without a cell; w mod 4: the dword tails of k_shear and the
resizes; ceil(w / 4) mod 64: the resize launcher's remainder wave) with several contents in turn on ONE pair of
handles, so that the counters a dense image left behind meet a featureless one and the reverse.  The mixed
batches put natural, noise, lattice, binary, coarse and featureless images, and pairs with an empty side, into
one enqueue, at both sides of the launchers' small / large batch rules, and force the shapes the rules did not
pick.  tests/test_sweep_cases_cpu.py shows that the inputs reach what they are meant to reach."""
import ctypes as C

import numpy as np
import pytest

import sweep_cases as S
from pyorbslam_amd._lib import call
from pyorbslam_amd.frame import stereo_match_arrays
from pyorbslam_amd.pyORBExtractor import ORBextractor

pytestmark = pytest.mark.gpu


# ---- the geometry sweep -------------------------------------------------------------------------------------
def _assert_pyramids(ex, ref, what):
    for l, (g, o) in enumerate(zip(ex.GetImagePyramid(sheared=False), ref.pyramid)):
        assert g.shape == o.shape and np.array_equal(g, o), (what, "level", l)
    for l, (g, o) in enumerate(zip(ex.GetImagePyramid(), ref.sheared)):
        assert g.shape == o.shape and np.array_equal(g, o), (what, "sheared level", l)


def _sweep_geometry(h, w, nlevels, resize_variants=False):
    """noise -> flat -> natural -> coarse on one pair of handles (right = left at disparity 3): keypoints,
    descriptors, both pyramids of both sides and the stereo result after every step."""
    prm = S.params(nlevels)
    exL, exR = ORBextractor(**prm), ORBextractor(**prm)
    ms = C.c_float()
    for name in S.CONTENT_ORDER:
        what = (h, w, name)
        left = S.content(name, 1000 * h + w, h, w)
        right = S.shifted(left, 3)
        refL, refR = S.ImageRef(left, nlevels), S.ImageRef(right, nlevels)
        kl, dl = exL.extract(left)
        kr, dr = exR.extract(right)
        S.assert_image(kl, dl, refL, what + ("left",))
        S.assert_image(kr, dr, refR, what + ("right",))
        _assert_pyramids(exL, refL, what + ("left",))
        _assert_pyramids(exR, refR, what + ("right",))
        res = stereo_match_arrays(exL, exR, S.BF, np.float32(S.FX))
        if name == "flat":  # as the reference: no keypoint, a released descriptor Mat, empty lists
            assert len(refL.kps) == 0 and len(kl) == 0 and len(kr) == 0, what
            assert dl.shape == (0, 0) and dr.shape == (0, 0), what
            assert all(len(res[k]) == 0 for k in ("u_right", "depth", "status", "match_r")), what
        else:
            assert len(kl) > 0 and len(kr) > 0, what
            S.assert_stereo(res, kl, S.PairRef(refL, refR), what)
        if resize_variants:
            # orbfe_microbench stage 0: 7 = the per-level launches, 5 = without the remainder wave, 6 = the cascade
            for variant in (7, 5, 6):
                call("orbfe_microbench", exL.handle, 0, variant, 1, C.byref(ms))
                _assert_pyramids(exL, refL, what + ("resize variant", variant))


@pytest.mark.parametrize("height", [96, 97])
def test_width_sweep(height):
    """36 consecutive widths from 96, 3 levels: every w mod 30, w mod 4 and (with both heights) W*H mod 4."""
    geos = [g for g in S.WIDTHS if g[0] == height]
    assert len(geos) == 36
    for h, w, nlevels in geos:
        _sweep_geometry(h, w, nlevels)


@pytest.mark.parametrize("width", [130, 131])
def test_height_sweep(width):
    """36 consecutive heights from 62, 4 levels: from level 0 alone having FAST cells (the other levels are
    still resized and sheared) to keypoints on three levels."""
    geos = [g for g in S.HEIGHTS if g[1] == width]
    assert len(geos) == 36
    for h, w, nlevels in geos:
        _sweep_geometry(h, w, nlevels)


@pytest.mark.parametrize("geo", S.RESIZE_TAILS, ids=lambda g: f"w{g[1]}")
def test_resize_tail_sweep(geo):
    """Level-1 widths with ceil(w / 4) mod 64 = 0, 1, 39, 40, 63 (launch_resize takes the remainder wave for
    1 .. 39): the automatic resize, and the per-level launches with and without the remainder wave and the
    cascade forced, each against the oracle's pyramid."""
    _sweep_geometry(*geo, resize_variants=True)


# ---- mixed batches ------------------------------------------------------------------------------------------
SMALL_PAIRS = 8
# ncells = 9 and kp_cap > 300 at the three geometries: 2P * ceil(9 / 4) >= 2048 from P = 342 (asserted below)
LARGE_PAIRS = 344
SHORT_PAIRS = 3


def _front_end(h, w, n_pairs):
    from pyorbslam_amd.batch import StereoFrontEnd
    return StereoFrontEnd(w, h, max_pairs=n_pairs, lanes=1, **S.params(S.MIXED_NLEVELS))


def _check_batch(fe, mb, n_pairs, what):
    """Every image and every pair of the batch against the oracle and the restatement, match_r included."""
    assert fe.overflow() == 0, what
    for p in range(n_pairs):
        kl, dl = fe.fetch_image(2 * p)
        kr, dr = fe.fetch_image(2 * p + 1)
        S.assert_image(kl, dl, mb.image_refs[2 * p], (what, "pair", p, mb.kinds[p], "left"))
        S.assert_image(kr, dr, mb.image_refs[2 * p + 1], (what, "pair", p, mb.kinds[p], "right"))
        S.assert_stereo(fe.fetch_stereo(p), kl, mb.pair_refs[p], (what, "pair", p, mb.kinds[p]))


def _detect_cells(fe, n_images):
    st = (C.c_int64 * 3)()
    call("orbfe_debug_detect_stats", fe.handle, st)
    assert st[0] > 0 and st[0] % n_images == 0, list(st)
    return st[0] // n_images


@pytest.mark.parametrize("n_pairs", [SMALL_PAIRS, LARGE_PAIRS], ids=["small", "large"])
@pytest.mark.parametrize("hw", S.MIXED_GEOMETRIES, ids=lambda hw: f"{hw[1]}x{hw[0]}")
def test_mixed_batch_in_every_launch_shape(hw, n_pairs):
    """One enqueue of the 8 pair kinds in turn (natural, noise, lattice, binary, coarse, empty left, empty right,
    both empty), below and above the launchers' batch-size rules; then every forced shape of detect, octree and
    describe with the later stages re-run in their automatic shape, everything re-checked after each; then a
    3-pair batch of other content on the same handle."""
    torch = pytest.importorskip("torch")
    h, w = hw
    mb = S.mixed_batch(h, w, n_pairs)
    fe = _front_end(h, w, n_pairs)
    dev = torch.from_numpy(mb.images).cuda()
    fe.enqueue(dev, n_pairs, bf=S.BF, fx=S.FX)
    _check_batch(fe, mb, n_pairs, "batch")
    assert any((r.status == 1).any() for r in mb.pair_refs) and any((r.status == 2).any() for r in mb.pair_refs)

    # which shapes the launchers' own rules picked for this batch (the launch_* of orbfe_resize.hip,
    # orbfe_detect.hip and orbfe_kernels.hip): k_resize_rows,
    # k_octree_bins<256> and k_stereo_bucket<256> from n_images >= kSmallBatchImages (32); detect_cpw: four cells
    # per wave from n_images * ceil(ncells / 4) >= 8 * 256 as well; orb_kpw: 8 keypoints per wave from
    # n_images * sum over levels of ceil(level kp_cap / 8) >= 16 * 256, which n_images * kp_cap / 8 implies
    n_images = 2 * n_pairs
    ncells = _detect_cells(fe, n_images)
    large = (n_images >= 32, n_images * ((ncells + 3) // 4) >= 8 * 256, n_images * fe.kp_cap // 8 >= 16 * 256)
    if n_pairs == LARGE_PAIRS:
        assert all(large), (n_images, ncells, fe.kp_cap)
    else:
        assert not any(large), (n_images, ncells, fe.kp_cap)
    _check_batch(fe, mb, n_pairs, "after the detect counters' run")

    ms = C.c_float()
    # detect 4 / 1 cells per wave, octree 256 / 512 threads, describe 8 / 4 / 2 keypoints per wave
    for stage, variant in [(1, 4), (1, 5), (2, 1), (2, 2), (3, 1), (3, 9), (3, 2)]:
        call("orbfe_microbench", fe.handle, stage, variant, 1, C.byref(ms))
        for later in range(stage + 1, 5):
            call("orbfe_microbench", fe.handle, later, 0, 1, C.byref(ms))
        _check_batch(fe, mb, n_pairs, ("forced", stage, variant))

    # a shorter batch after the full one: what the pairs beyond it left behind must not leak into pairs 0 .. 2,
    # whose slots go dense -> other dense, dense -> empty left, dense -> empty right
    short = S.mixed_batch(h, w, SHORT_PAIRS, 5000, 4)
    assert short.kinds == ["coarse", "flat_noise", "noise_flat"]
    fe.enqueue(torch.from_numpy(short.images).cuda(), SHORT_PAIRS, bf=S.BF, fx=S.FX)
    _check_batch(fe, short, SHORT_PAIRS, "short batch after the full one")
    fe.enqueue(dev, n_pairs, bf=S.BF, fx=S.FX)
    _check_batch(fe, mb, n_pairs, "full batch after the short one")


@pytest.mark.parametrize("hw", [g for g in S.MIXED_GEOMETRIES if (g[0] * g[1]) % 2 == 0],
                         ids=lambda hw: f"{hw[1]}x{hw[0]}")
def test_mixed_batch_from_a_misaligned_base(hw):
    """W*H = 0 and 2 mod 4 never move an image off a dword boundary by themselves; here the batch starts 1, 2 and
    3 bytes into a buffer.  The results equal the aligned run's, which equals the oracle."""
    torch = pytest.importorskip("torch")
    h, w = hw
    n = SMALL_PAIRS
    mb = S.mixed_batch(h, w, n)
    nbytes = mb.images.size
    fe = _front_end(h, w, n)
    buf = torch.zeros(nbytes + 3, dtype=torch.uint8, device="cuda")
    host = torch.from_numpy(mb.images.reshape(-1))
    results = []
    for offset in (0, 1, 2, 3):
        view = buf[offset:offset + nbytes]
        view.copy_(host)
        images = view.view(2 * n, h, w)
        assert images.is_contiguous() and images.data_ptr() == buf.data_ptr() + offset
        assert buf.data_ptr() % 4 == 0
        fe.enqueue(images, n, bf=S.BF, fx=S.FX)
        _check_batch(fe, mb, n, ("offset", offset))
        results.append(([fe.fetch_image(i) for i in range(2 * n)], [fe.fetch_stereo(p) for p in range(n)]))
    for offset, (imgs, pairs) in enumerate(results[1:], 1):
        for i, ((k0, d0), (k1, d1)) in enumerate(zip(results[0][0], imgs)):
            assert k0.tobytes() == k1.tobytes() and np.array_equal(d0, d1), (offset, i)
        for p, (s0, s1) in enumerate(zip(results[0][1], pairs)):
            assert all(np.array_equal(s0[k], s1[k]) for k in s0), (offset, p)


@pytest.mark.parametrize("compact", [False, True])
def test_mixed_batch_records(compact):
    """k_pack / k_pack_compact over the mixed batch: every record, those of empty images included, decodes to
    what orbfe_batch_fetch / _fetch_stereo return (which the tests above compare with the oracle)."""
    torch = pytest.importorskip("torch")
    from pyorbslam_amd import dist as D
    h, w = S.MIXED_GEOMETRIES[0]
    n = SMALL_PAIRS
    mb = S.mixed_batch(h, w, n)
    fe = _front_end(h, w, n)
    fe.enqueue(torch.from_numpy(mb.images).cuda(), n, bf=S.BF, fx=S.FX)
    rb = (D.compact_record_bytes if compact else D.record_bytes)(fe.kp_cap)
    buf = torch.full((n, rb), 0xA5, dtype=torch.uint8, device="cuda")
    D.pack_device([fe], [n], buf, compact)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    for p in range(n):
        u = D.unpack_compact(fe.kp_cap, host[p], fe.scales) if compact else D.unpack(fe.kp_cap, host[p])
        kl, dl = fe.fetch_image(2 * p)
        kr, dr = fe.fetch_image(2 * p + 1)
        s = fe.fetch_stereo(p)
        what = (p, mb.kinds[p])
        assert len(u["kps_left"]) == len(mb.image_refs[2 * p].kps), what
        assert len(u["kps_right"]) == len(mb.image_refs[2 * p + 1].kps), what
        assert u["kps_left"].tobytes() == kl.tobytes() and u["kps_right"].tobytes() == kr.tobytes(), what
        assert np.array_equal(u["desc_left"], dl) and np.array_equal(u["desc_right"], dr), what
        for k in ("u_right", "depth", "status"):
            assert np.array_equal(u[k], s[k]), what + (k,)
