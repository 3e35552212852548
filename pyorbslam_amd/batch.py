"""Batched-frames front-end: extract + stereo-match many device-resident stereo pairs per enqueue.

This is the throughput path of BASELINE.json (stereo pairs/s): images (2P, H, W) uint8 already in HBM
(a torch tensor on the GPU), pair p = images (2p, 2p+1) = (left, right).  One call enqueues the whole
pipeline (7 resize launches, detect, octree, describe, stereo) on the given HIP stream; results stay on
the device until fetched.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KP_DTYPE, BatchView, BowMatchOut, BowOut, call, ptr

KITTI_BF = 386.1448  # KITTI00-02.yaml Camera.bf
KITTI_FX = 718.856   # KITTI00-02.yaml Camera.fx
# EuRoC MAV rectified stereo (ORB-SLAM2 EuRoC.yaml Camera.bf, Camera.fx; the reference ships KITTI settings
# only), the EuRoC case of tests/test_gpu_stereo.py
EUROC_BF = 47.90639384423901
EUROC_FX = 435.2046959714599


def camera_constants(width: int, height: int) -> tuple[float, float]:
    """(bf, fx) of the camera whose image size this is: EuRoC for 752x480, KITTI otherwise."""
    return (EUROC_BF, EUROC_FX) if (int(width), int(height)) == (752, 480) else (KITTI_BF, KITTI_FX)


class StereoFrontEnd:
    def __init__(self, width: int = 1241, height: int = 376, max_pairs: int = 64, nfeatures: int = 2000,
                 scaleFactor: float = 1.2, nlevels: int = 8, iniThFAST: int = 20, minThFAST: int = 7,
                 resize_simd_lanes: int = 16, lanes: int = 4, graphs: bool = False):
        self.width, self.height, self.max_pairs = int(width), int(height), int(max_pairs)
        self._params = _lib.make_params(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, resize_simd_lanes)
        h = C.c_void_p()
        call("orbfe_create", C.byref(self._params), C.byref(h))
        self._h = h
        call("orbfe_batch_reserve", h, self.width, self.height, 2 * self.max_pairs)
        # concurrent chunks of enqueue() on internal streams (results are independent of it)
        call("orbfe_set_lanes", h, int(lanes))
        # graphs=True: one-lane enqueues replay a captured HIP graph (orbfe_set_graphs ORBFE_GRAPH_BATCH; off by
        # default: graph launches on several streams serialise the handles' chains; results do not depend on it)
        if _lib.has("orbfe_set_graphs"):
            call("orbfe_set_graphs", h, 3 if graphs else 1)
        v = BatchView()
        call("orbfe_batch_view_get", h, C.byref(v))
        self.kp_cap = v.kp_cap
        self._bow, self._bow_frames = None, 0  # bow()'s device buffers, made on its first call
        self._bow_step, self._match = 1, None  # match_bow()'s outputs, made on its first call
        self.scales = np.zeros(int(nlevels), np.float32)  # the level scale factors (compact records)
        call("orbfe_get_scales", h, self.scales.ctypes.data_as(C.c_void_p), None, None, None, None)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib._lib is not None:
            _lib.lib().orbfe_destroy(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def enqueue(self, images, n_pairs: int | None = None, bf: float = KITTI_BF, fx: float = KITTI_FX,
                stream_ptr: int = 0) -> None:
        """images: device tensor (>= 2*n_pairs, H, W) uint8, C-contiguous.  stream_ptr: raw hipStream_t
        (torch.cuda.current_stream().cuda_stream), 0 = the null stream."""
        n_pairs = images.shape[0] // 2 if n_pairs is None else int(n_pairs)
        if images.dtype.itemsize != 1 or tuple(images.shape[1:]) != (self.height, self.width):
            raise ValueError("images must be (2P, H, W) uint8 with the reserved H, W")
        if not images.is_contiguous() or not images.is_cuda:
            raise ValueError("images must be a contiguous GPU tensor")
        if n_pairs > self.max_pairs or 2 * n_pairs > images.shape[0]:
            raise ValueError("n_pairs exceeds the reservation or the tensor")
        call("orbfe_frontend_batch_device", self._h, C.c_void_p(images.data_ptr()), self.width * self.height,
             n_pairs, float(bf), float(np.float32(fx)), C.c_void_p(stream_ptr))

    def enqueue_extract(self, images, n_images: int | None = None, stream_ptr: int = 0) -> None:
        n = images.shape[0] if n_images is None else int(n_images)
        call("orbfe_extract_batch_device", self._h, C.c_void_p(images.data_ptr()), self.width * self.height, n,
             C.c_void_p(stream_ptr))

    def graph_stats(self) -> dict:
        """HIP-graph captures and launches of this handle so far, and the graphs cached now."""
        cap, lau, n = C.c_int64(), C.c_int64(), C.c_int32()
        if not _lib.has("orbfe_graph_stats"):
            return {"captures": 0, "launches": 0, "cached": 0}
        call("orbfe_graph_stats", self._h, C.byref(cap), C.byref(lau), C.byref(n))
        return {"captures": cap.value, "launches": lau.value, "cached": n.value}

    def overflow(self) -> int:
        """Overflow word of the last batch (0 = no on-device capacity bound was hit); synchronises."""
        v = C.c_int32()
        call("orbfe_batch_status", self._h, C.byref(v))
        return v.value

    def bow(self, vocab, levels_up: int = 4, side: str = "left", stream_ptr: int = 0) -> int:
        """Enqueue the BoW and feature vectors of the last batch's images on stream_ptr (the stream the batch was
        enqueued on): orbfe_vocab_bow_device on the batch view's desc / count, nothing goes through the host.
        side="left": frame p is pair p's left image; "both": frame i is image i.  Returns the number of frames;
        fetch_bow(i) reads one.  Output and scratch buffers are allocated on the first call and kept."""
        import torch
        if side not in ("left", "both"):
            raise ValueError('side must be "left" or "both"')
        v = BatchView()
        call("orbfe_batch_view_get", self._h, C.byref(v))
        step = 2 if side == "left" else 1
        n_frames = v.n_images // step
        cap = self.kp_cap
        if self._bow is None:
            m = 2 * self.max_pairs
            need = C.c_int64()
            call("orbfe_vocab_bow_scratch_bytes", m, 2 * cap, C.byref(need))
            dev = torch.device("cuda", torch.cuda.current_device())
            ints = torch.zeros((4, m, cap), dtype=torch.int32, device=dev)    # bow_word, fv_node, fv_end, fv_idx
            per = torch.zeros((4, m), dtype=torch.int32, device=dev)          # n_words, n_nodes, n_kept, status
            weight = torch.zeros((m, cap), dtype=torch.float64, device=dev)
            scratch = torch.zeros(max(need.value, 8) // 8, dtype=torch.int64, device=dev)
            out = BowOut(n_words=per[0].data_ptr(), bow_word=ints[0].data_ptr(), bow_weight=weight.data_ptr(),
                         n_nodes=per[1].data_ptr(), fv_node=ints[1].data_ptr(), fv_end=ints[2].data_ptr(),
                         fv_idx=ints[3].data_ptr(), n_kept=per[2].data_ptr(), status=per[3].data_ptr())
            torch.cuda.synchronize()  # once: the fills above ran on torch's stream, the kernels run on stream_ptr
            self._bow = dict(ints=ints, per=per, weight=weight, scratch=scratch, out=out)
        b = self._bow
        self._bow_frames, self._bow_step = n_frames, step
        if n_frames:
            call("orbfe_vocab_bow_device", vocab._handle(), C.c_void_p(v.desc), step * cap, C.c_void_p(v.count), step,
                 n_frames, int(vocab.L - levels_up), cap, C.byref(b["out"]), C.c_void_p(b["scratch"].data_ptr()),
                 b["scratch"].numel() * 8, C.c_void_p(stream_ptr))
        return n_frames

    def train_vocabulary(self, k: int = 10, L: int = 5, weighting: str = "TF_IDF", scoring: str = "L1_NORM",
                         side: str = "left", seed: int = 0, max_iter: int = 64):
        """Train a vocabulary on the last batch's resident descriptors (orbfe_vocab_train with desc_on_device = 1 on
        the view bow() uses): image f is the first count[f] descriptors of its kp_cap slots.  side as in bow().  The
        counts are fetched to the host first, which synchronises the device.  Returns a TemplatedVocabulary ready
        for bow()."""
        from .vocabulary import TemplatedVocabulary
        if side not in ("left", "both"):
            raise ValueError('side must be "left" or "both"')
        v = BatchView()
        call("orbfe_batch_view_get", self._h, C.byref(v))
        step = 2 if side == "left" else 1
        n_frames = v.n_images // step
        if n_frames < 1:
            raise ValueError("no batch has been enqueued")
        count = np.zeros(v.n_images, np.int32)
        hip = _lib.lib()  # the HIP runtime the library is linked against
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        if hip.hipDeviceSynchronize() != 0 or hip.hipMemcpy(ptr(count), C.c_void_p(v.count), count.nbytes, 2) != 0:
            raise RuntimeError("reading the batch's counts from the device failed")  # 2: hipMemcpyDeviceToHost
        count = np.clip(count[::step], 0, self.kp_cap).astype(np.int32)
        start = np.arange(n_frames, dtype=np.int64) * (step * self.kp_cap)
        voc = TemplatedVocabulary(k, L, weighting, scoring)
        return voc.train_arrays(v.desc, True, start, count, seed, max_iter)

    def fetch_bow(self, i: int):
        """vocabulary.BowArrays of frame i of the last bow(); synchronises the device."""
        import torch
        from .vocabulary import BowArrays
        if self._bow is None or not 0 <= int(i) < self._bow_frames:
            raise IndexError("no such frame in the last bow()")
        torch.cuda.synchronize()
        b, i = self._bow, int(i)
        nw, nn, nk, _ = b["per"][:, i].tolist()
        ints = b["ints"][:, i, :max(nw, nn, nk)].cpu().numpy()
        return BowArrays(ints[0, :nw].copy(), b["weight"][i, :nw].cpu().numpy(), ints[1, :nn].copy(),
                         ints[2, :nn].copy(), ints[3, :nk].copy(), nk)

    def query_bow(self, db, gate_ratio: float = 0.8, exclude=None, hit_cap=None, stream_ptr: int = 0,
                  dense: bool = False):
        """Ask the place-recognition database db (kfdb.BowDatabase) with every frame of the last bow(), on
        stream_ptr (the stream bow() ran on): orbfe_kfdb_query_many_device reads the resident BoW vectors where
        bow() left them, scores all frames against all slots in one launch, applies the word gate
        common > int(max_common * gate_ratio) per frame on the device and brings back the surviving slots only.
        exclude: per frame an iterable of slots (or None) that neither set the gate nor are reported, e.g. the
        slots of the frame's temporal neighbours.  Returns one record per frame (kfdb.run_many): n_sharing,
        max_common, n_hits and the hits' slot / common / first / score in ascending slot order; a frame without
        words gets an empty record.  Synchronises stream_ptr."""
        from .kfdb import run_many
        if self._bow is None:
            raise RuntimeError("query_bow needs the BoW vectors of a bow() call first")
        n, out = self._bow_frames, self._bow["out"]

        def launch(excl_off, excl_slot, ratio, cap, stride, res):
            return _lib.lib().orbfe_kfdb_query_many_device(db._h, C.byref(out), self.kp_cap, n, excl_off, excl_slot,
                                                           ratio, cap, stride, res, C.c_void_p(stream_ptr))

        return run_many(db, n, launch, gate_ratio, exclude, hit_cap, dense)

    def match_bow(self, pairs, th: int = 50, inclusive: bool = False, nnratio: float = 1.0, eligible=None,
                  stream_ptr: int = 0) -> int:
        """Enqueue the BoW-guided match (k_bow_match, ORBMatcher.py:21-213 before the rotation rejection) of frame
        pairs of the last bow() on stream_ptr (the stream bow() ran on): orbfe_bow_match_device on the batch view's
        desc / kps and bow()'s resident feature vectors.  pairs: (P, 2) frame indices of that bow() (with
        side="left" frame p is pair p's left image).  eligible: None (every feature), "stereo" (side="left" only:
        the features with a stereo match, the pair's status array, on both sides) or an (n_frames, kp_cap) mask
        used for both sides.  Returns P; fetch_bow_matches(p) reads one pair.  The outputs are allocated on the
        first call and kept (and grown when a later call brings more pairs)."""
        import torch
        if self._bow is None or not self._bow_frames:
            raise RuntimeError("match_bow needs the feature vectors of a bow() call first")
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n_pairs, cap, step = len(pairs), self.kp_cap, self._bow_step
        v = BatchView()
        call("orbfe_batch_view_get", self._h, C.byref(v))
        dev = torch.device("cuda", torch.cuda.current_device())
        own_stream = stream_ptr != torch.cuda.current_stream().cuda_stream
        elig_ptr, elig_stride, mask = None, 0, None
        if isinstance(eligible, str):
            if eligible != "stereo" or step != 2:
                raise ValueError('eligible="stereo" needs bow(side="left")')
            elig_ptr, elig_stride = C.c_void_p(v.status), cap
        elif eligible is not None:
            m = np.ascontiguousarray(eligible).astype(np.uint8, copy=False)
            if m.shape != (self._bow_frames, cap):
                raise ValueError("eligible must be (n_frames, kp_cap)")
            mask = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
            elig_ptr, elig_stride = C.c_void_p(mask.data_ptr()), cap
        mt = self._match
        if mt is None or mt["cap_pairs"] < n_pairs:
            cp = max(n_pairs, 2 * self.max_pairs)
            mt = dict(cap_pairs=cp, ints=torch.zeros((2, cp, cap), dtype=torch.int32, device=dev),
                      bins=torch.zeros((cp, cap), dtype=torch.int8, device=dev),
                      hist=torch.zeros((cp, 32), dtype=torch.int32, device=dev),
                      n_raw=torch.zeros(cp, dtype=torch.int32, device=dev),
                      pairs=torch.zeros((cp, 2), dtype=torch.int32, device=dev))
            mt["out"] = BowMatchOut(match12=mt["ints"][0].data_ptr(), match21=mt["ints"][1].data_ptr(),
                                    bin12=mt["bins"].data_ptr(), hist=mt["hist"].data_ptr(),
                                    n_raw=mt["n_raw"].data_ptr(), status=self._bow["per"][3].data_ptr())
            self._match = mt
            own_stream = True
        mt["host_pairs"], mt["n_pairs"], mt["mask"] = pairs.copy(), n_pairs, mask
        if n_pairs:
            mt["pairs"][:n_pairs].copy_(torch.from_numpy(pairs))
            if own_stream:  # the fills and the upload ran on torch's stream, the kernel runs on stream_ptr
                torch.cuda.current_stream().synchronize()
            call("orbfe_bow_match_device", C.c_void_p(v.desc), step * cap, C.c_void_p(v.count), step, self._bow_frames,
                 C.c_void_p(v.kps + KP_DTYPE.fields["angle"][1]), KP_DTYPE.itemsize // 4, elig_ptr, elig_stride,
                 elig_ptr, elig_stride, C.byref(self._bow["out"]), cap, C.c_void_p(mt["pairs"].data_ptr()), n_pairs,
                 int(th), int(bool(inclusive)), float(nnratio), C.byref(mt["out"]), cap, C.c_void_p(stream_ptr))
        return n_pairs

    def fetch_bow_matches(self, p: int, check_orientation: bool = True):
        """(match12, match21, n) of pair p of the last match_bow(): match12[i1] = i2 or -1 over frame 1's features,
        match21 the inverse over frame 2's, n the matches left after the reference's rotation rejection (the
        three fullest bins by ORBMatcher.compute_three_maxima, on the host; check_orientation=False keeps every
        match).  Synchronises the device."""
        import torch
        from .matcher import ORBMatcher
        mt = self._match
        if mt is None or not 0 <= int(p) < mt["n_pairs"]:
            raise IndexError("no such pair in the last match_bow()")
        torch.cuda.synchronize()
        p = int(p)
        n = C.c_int32()
        lens = []
        for f in mt["host_pairs"][p].tolist():
            k = 0
            if 0 <= f < self._bow_frames:
                call("orbfe_batch_fetch", self._h, f * self._bow_step, None, None, self.kp_cap, C.byref(n))
                k = min(n.value, self.kp_cap)
            lens.append(k)
        m12 = mt["ints"][0, p, :lens[0]].cpu().numpy()
        m21 = mt["ints"][1, p, :lens[1]].cpu().numpy()
        b12 = mt["bins"][p, :lens[0]].cpu().numpy()
        return ORBMatcher(1.0, bool(check_orientation))._bow_reject(m12, m21, b12, mt["hist"][p].cpu().numpy(),
                                                                    int(mt["n_raw"][p]))

    def bow_status(self) -> int:
        """OR of the ORBFE_BOW_* flags of every bow() and match_bow() so far (0: no count was clamped, no pair named
        a missing frame); synchronises."""
        import torch
        if self._bow is None:
            return 0
        torch.cuda.synchronize()
        return int(self._bow["per"][3, 0])

    def fetch_image(self, i: int) -> tuple[np.ndarray, np.ndarray]:
        kps = np.empty(self.kp_cap, KP_DTYPE)
        desc = np.empty((self.kp_cap, 32), np.uint8)
        n = C.c_int32()
        call("orbfe_batch_fetch", self._h, int(i), ptr(kps), ptr(desc), self.kp_cap, C.byref(n))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def fetch_stereo(self, p: int) -> dict:
        u = np.empty(self.kp_cap, np.float32)
        d = np.empty(self.kp_cap, np.float32)
        st = np.empty(self.kp_cap, np.int8)
        m = np.empty(self.kp_cap, np.int32)
        n = C.c_int32()
        call("orbfe_batch_fetch_stereo", self._h, int(p), ptr(u), ptr(d), ptr(st), ptr(m), self.kp_cap, C.byref(n))
        k = n.value
        return dict(u_right=u[:k].copy(), depth=d[:k].copy(), status=st[:k].copy(), match_r=m[:k].copy())
