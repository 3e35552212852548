"""The stereo matcher at the boundaries of its gates, against the REFERENCE's own outputs, on every launch path.

tests/golden/stereo_edges_*.npz hold what the reference's Frame.compute_stereo_matches returns for the cases of
tests/stereo_cases.py: tiny pairs (97 x 131, 3 levels) at which `minU <= uR`, `disparity < maxD`, the 74 / 75
descriptor threshold, a SAD minimum at the ends of its scan, first-minimum ties of both searches, negative and
zero disparities, window rows that leave the level, empty row buckets and row buckets of more than 64 and 96
entries all decide results (tests/test_stereo_cases_cpu.py counts them).  Status, u_right and depth are compared
through to_reference_lists and encode, bit for bit and without tolerance; match_r against the restatement.
Every case runs through orbfe_stereo_match (separate calls), the frame path, one batch enqueue with fewer than
32 images and one with more, the latter from an aligned and from an odd base address.

The tall geometries (879 and 880 rows x 480) run the row buckets at the first height above the describe kernel's
per-wave H buffer: the front-end still builds them inside the describe launch there (all four waves' buffers hold
the counters, up to 3 519 rows; orbfe_get_stereo_bucket_kernel reports it), and the separate bucket kernel is
reached at both of its workgroup sizes through orbfe_stereo_match and orbfe_stereo_batch_device."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import stereo_cases as SC
from oracle import stereo_oracle
from pyorbslam_amd._lib import call
from pyorbslam_amd.frame import stereo_match_arrays, to_reference_lists
from pyorbslam_amd.pyORBExtractor import ORBextractor

pytestmark = pytest.mark.gpu


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _assert_inputs(kl, dl, kr, dr, group):
    """Inputs identical to those the reference was fed (extractor parity), before any result is compared."""
    g = SC.load_golden(group)
    assert _sha(kl) == str(g["kps_left_sha"]) and _sha(dl) == str(g["desc_left_sha"]), group
    assert _sha(kr) == str(g["kps_right_sha"]) and _sha(dr) == str(g["desc_right_sha"]), group


def _assert_result(res, kl, bf, want, match_r, what):
    u, d = to_reference_lists(res, kl, bf)
    su, vu = stereo_oracle.encode(u)
    sd, vd = stereo_oracle.encode(d)
    status, u_right, depth = want
    bad = np.flatnonzero(su != status)
    assert bad.size == 0, (what, f"{bad.size} status mismatches, first {bad[:5]}: gpu {su[bad[:5]]} ref {status[bad[:5]]}")
    assert np.array_equal(sd, status), what
    assert np.array_equal(vu, u_right) and np.array_equal(vd, depth), what
    assert np.array_equal(res["match_r"], match_r), what


def _assert_case(res, kl, case, what):
    g = SC.golden_of(case)
    _assert_result(res, kl, case.bf, (g["status"], g["u_right"], g["depth"]), SC.restated(case.id)[3], (case.id, what))


def _bucket_kernel(handle, n_images):
    fused, threads = C.c_int32(-1), C.c_int32(-1)
    call("orbfe_get_stereo_bucket_kernel", handle, n_images, C.byref(fused), C.byref(threads))
    return fused.value, threads.value


# ---- the boundary cases: separate calls and the frame path ----------------------------------------------------
@pytest.mark.parametrize("group", SC.GROUPS)
def test_separate_calls_match_reference_golden(group):
    """Two extractions and orbfe_stereo_match (the separate k_stereo_bucket<1024>), every fx of the pair."""
    cases = SC.cases_of(group)
    left, right = SC.make_pair(cases[0].pair)
    exL, exR = ORBextractor(**cases[0].params), ORBextractor(**cases[0].params)
    kl, dl = exL.extract(left)
    kr, dr = exR.extract(right)
    _assert_inputs(kl, dl, kr, dr, group)
    assert _bucket_kernel(exL.handle, 2) == (1, 1024)
    for case in cases:
        _assert_case(stereo_match_arrays(exL, exR, case.bf, np.float32(case.fx)), kl, case, "separate calls")


@pytest.mark.parametrize("group", SC.GROUPS)
def test_frame_path_matches_reference_golden(group):
    """operator_kd_stereo (orbfe_frame_extract: one enqueue, the row buckets inside the describe launch)."""
    cases = SC.cases_of(group)
    left, right = SC.make_pair(cases[0].pair)
    exL, exR = ORBextractor(**cases[0].params), ORBextractor(**cases[0].params)
    for case in cases:
        kl, dl, kr, dr = exL.operator_kd_stereo(left, right, exR, case.bf, np.float32(case.fx), want_pyramid=False)
        _assert_inputs(kl, dl, kr, dr, group)
        _assert_case(exL.stereo_result, kl, case, "frame path")


# ---- the boundary cases in batches ----------------------------------------------------------------------------
def _front_end(params, h, w, n_pairs):
    from pyorbslam_amd.batch import StereoFrontEnd
    return StereoFrontEnd(w, h, max_pairs=n_pairs, lanes=1, **params)


def _batch_images(groups, repeat):
    pairs = [SC.make_pair(SC.cases_of(g)[0].pair) for g in groups] * repeat
    return np.ascontiguousarray(np.stack([im for p in pairs for im in p]))


def _device_images(torch, host, offset):
    """The batch on the device, starting `offset` bytes into a 4-byte aligned buffer."""
    buf = torch.zeros(host.size + 4, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    view = buf[offset:offset + host.size]
    view.copy_(torch.from_numpy(host.reshape(-1)))
    images = view.view(*host.shape)
    assert images.is_contiguous() and images.data_ptr() % 4 == offset % 4
    return buf, images


def _run_batches(groups, repeat, offset, fxs):
    torch = pytest.importorskip("torch")
    params = SC.cases_of(groups[0])[0].params
    host = _batch_images(groups, repeat)
    n_pairs = len(groups) * repeat
    fe = _front_end(params, SC.H, SC.W, n_pairs)
    keep, images = _device_images(torch, host, offset)
    fused, threads = _bucket_kernel(fe.handle, 2 * n_pairs)
    assert fused == 1 and threads == (1024 if 2 * n_pairs < 32 else 256)
    for fx in fxs:  # one enqueue per fx on the same handle
        fe.enqueue(images, n_pairs, bf=SC.BF, fx=fx)
        assert fe.overflow() == 0
        for p in range(n_pairs):
            group = groups[p % len(groups)]
            case = next(c for c in SC.cases_of(group) if c.fx == fx)
            kl, dl = fe.fetch_image(2 * p)
            kr, dr = fe.fetch_image(2 * p + 1)
            _assert_inputs(kl, dl, kr, dr, group)
            _assert_case(fe.fetch_stereo(p), kl, case, ("batch", n_pairs, "pair", p, "offset", offset))
    del keep


PAIR_GROUPS = list(SC.PAIRS)  # the nfeatures = 300 handle: 10 pairs


def test_batch_below_32_images_matches_reference_golden():
    """All pairs once: 20 images, the small-batch launch shapes."""
    assert 2 * len(PAIR_GROUPS) < 32
    _run_batches(PAIR_GROUPS, 1, 0, SC.FXS)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
def test_batch_from_32_images_matches_reference_golden(offset):
    """All pairs twice: 40 images, the large-batch launch shapes; W * H is odd, so every second image starts at
    an odd address from the aligned base and every other one from the odd base."""
    assert 2 * 2 * len(PAIR_GROUPS) >= 32 and (SC.H * SC.W) % 2 == 1
    _run_batches(PAIR_GROUPS, 2, offset, SC.FXS)


@pytest.mark.parametrize("repeat,offset", [(1, 0), (16, 0), (16, 1)], ids=["once", "x16-aligned", "x16-odd"])
def test_long_buckets_in_batches_match_reference_golden(repeat, offset):
    """nfeatures = 1000 on its own handle: row buckets of 65 .. 109 entries, the third and fourth step of the
    candidate loop with its prefetched slots, as 2 and as 32 images."""
    _run_batches(["noise3_n1000"], repeat, offset, [c.fx for c in SC.LONG_CASES])


# ---- the tall geometries --------------------------------------------------------------------------------------
def _tall_images(h, n_pairs):
    imgs = []
    for p in range(n_pairs):
        left, right, _ = SC.tall_pair(h, p % len(SC.TALL_SEEDS))
        imgs += [left.image, right.image]
    return np.ascontiguousarray(np.stack(imgs))


def _assert_tall_image(kps, desc, ref, what):
    assert kps.tobytes() == ref.kps.tobytes() and np.array_equal(np.asarray(desc).reshape(-1, 32), ref.desc), what


def _assert_tall_batch(fe, h, n_pairs, what):
    assert fe.overflow() == 0, what
    for p in range(n_pairs):
        left, right, (status, u_right, depth, match_r) = SC.tall_pair(h, p % len(SC.TALL_SEEDS))
        kl, dl = fe.fetch_image(2 * p)
        kr, dr = fe.fetch_image(2 * p + 1)
        _assert_tall_image(kl, dl, left, (what, p, "left"))
        _assert_tall_image(kr, dr, right, (what, p, "right"))
        _assert_result(fe.fetch_stereo(p), kl, SC.BF, (status, u_right, depth), match_r, (what, "pair", p))


@pytest.mark.parametrize("h", SC.TALL_HEIGHTS)
def test_tall_geometry_single_paths(h):
    """Separate calls (k_stereo_bucket<1024> over 880 / 881 row counters) and the frame path, both pairs."""
    exL, exR = ORBextractor(**SC.TALL_PARAMS), ORBextractor(**SC.TALL_PARAMS)
    for k in range(len(SC.TALL_SEEDS)):
        left, right, (status, u_right, depth, match_r) = SC.tall_pair(h, k)
        kl, dl = exL.extract(left.image)
        kr, dr = exR.extract(right.image)
        _assert_tall_image(kl, dl, left, (h, k, "left"))
        _assert_tall_image(kr, dr, right, (h, k, "right"))
        # more than one wave's H buffer (880 counters) but all four waves' hold them: still inside k_orb
        assert _bucket_kernel(exL.handle, 2) == (1, 1024)
        res = stereo_match_arrays(exL, exR, SC.BF, np.float32(100.0))
        _assert_result(res, kl, SC.BF, (status, u_right, depth), match_r, (h, k, "separate calls"))
    fL, fR = ORBextractor(**SC.TALL_PARAMS), ORBextractor(**SC.TALL_PARAMS)
    for k in range(len(SC.TALL_SEEDS)):
        left, right, (status, u_right, depth, match_r) = SC.tall_pair(h, k)
        kl, dl, kr, dr = fL.operator_kd_stereo(left.image, right.image, fR, SC.BF, np.float32(100.0), want_pyramid=False)
        _assert_tall_image(kl, dl, left, (h, k, "frame left"))
        _assert_tall_image(kr, dr, right, (h, k, "frame right"))
        _assert_result(fL.stereo_result, kl, SC.BF, (status, u_right, depth), match_r, (h, k, "frame path"))


@pytest.mark.parametrize("n_pairs,threads", [(2, 1024), (16, 256)], ids=["2-pairs", "16-pairs"])
@pytest.mark.parametrize("h", SC.TALL_HEIGHTS)
def test_tall_geometry_batches(h, n_pairs, threads):
    """The front-end enqueue (row buckets inside the describe launch), and on a fresh handle the separate
    extraction and stereo calls, whose k_stereo_bucket runs 1 024 threads for 4 images and 256 for 32; the fresh
    handle's bucket buffers hold nothing before, so a bucket kernel that did not run cannot pass."""
    torch = pytest.importorskip("torch")
    images = torch.from_numpy(_tall_images(h, n_pairs)).cuda()
    params = {k: v for k, v in SC.TALL_PARAMS.items()}
    fe = _front_end(params, h, SC.TALL_W, n_pairs)
    assert _bucket_kernel(fe.handle, 2 * n_pairs) == (1, threads)
    assert _bucket_kernel(fe.handle, 31)[1] == 1024 and _bucket_kernel(fe.handle, 32)[1] == 256
    fe.enqueue(images, n_pairs, bf=SC.BF, fx=100.0)
    _assert_tall_batch(fe, h, n_pairs, (h, n_pairs, "front-end"))
    sep = _front_end(params, h, SC.TALL_W, n_pairs)
    sep.enqueue_extract(images, 2 * n_pairs)
    call("orbfe_stereo_batch_device", sep.handle, n_pairs, SC.BF, float(np.float32(100.0)), None)
    _assert_tall_batch(sep, h, n_pairs, (h, n_pairs, "separate batch calls"))
