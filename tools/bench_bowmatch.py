"""What k_bow_match buys: the BoW-guided match of many frame pairs in one launch.

  1. host drop-ins: a loop of N ORBMatcher.search_by_BoW_kf_kf calls (one k_hamming_search launch and a Python
     replay each; still in the tree, so it is the baseline) against one search_by_BoW_kf_kf_many call, on a
     tests/matcher_world world of `--feats` features per keyframe, N in --cands; the many call's host
     conversion and kernel time are reported beside it;
  2. device path: k_bow_match over P pairs of consecutive left images of a KITTI-sized batch that already went
     through enqueue() and bow(), by HIP events on the launch stream, P in --pairs, with bow()'s time beside it.
     Frame i is image i // 4 of a seeded synthetic set shifted by 3 * (i % 4) pixels, so consecutive frames
     share features as consecutive video frames do.

Every measurement is taken --rounds times, the variants alternating inside a round; the JSON holds every
sample.  --device-only runs part 2 alone (the shape to put under a kernel trace).

  python tools/bench_bowmatch.py [--rounds 3] [--cands 1 4 16] [--pairs 1 64 512] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


class _Z:
    def __init__(self, d):
        self._d, self.files = d, list(d.keys())

    def __getitem__(self, k):
        return self._d[k]


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4),
            "samples": [round(x, 4) for x in xs]}


def host_part(a):
    import matcher_world as MW
    from pyorbslam_amd import _lib, matcher
    rng = np.random.Generator(np.random.PCG64(11))
    n_max = max(a.cands)
    w = MW.build(_Z(MW.make_world(rng, n_kf=n_max + 1, n=a.feats, n_mp=int(a.feats * 0.7), n_words=a.feats // 15)))
    m = matcher.ORBMatcher(0.75, True)
    out = {}
    for n in a.cands:
        kfs = w.kfs[1:1 + n]
        want = [m.search_by_BoW_kf_kf(w.kfs[0], kf) for kf in kfs]  # warm-up of both, and one result
        got = m.search_by_BoW_kf_kf_many(w.kfs[0], kfs)
        assert all(x[0] == y[0] and all(p is q for p, q in zip(x[1], y[1])) for x, y in zip(got, want))
        loop, many, conv, kern = [], [], [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for kf in kfs:
                m.search_by_BoW_kf_kf(w.kfs[0], kf)
            t1 = time.perf_counter()
            m.search_by_BoW_kf_kf_many(w.kfs[0], kfs)
            t2 = time.perf_counter()
            ms = C.c_float()
            _lib.call("orbfe_bow_match_last_ms", C.byref(ms))
            for kf in [w.kfs[0]] + kfs:
                matcher._bow_frame(kf, kf.mvKeysUn, kf.get_map_point_matches())
            t3 = time.perf_counter()
            loop.append((t1 - t0) * 1e3)
            many.append((t2 - t1) * 1e3)
            conv.append((t3 - t2) * 1e3)
            kern.append(ms.value)
        out[str(n)] = {"loop_ms": spread(loop), "many_ms": spread(many), "many_object_to_array_ms": spread(conv),
                       "many_kernel_ms": spread(kern), "matches": [g[0] for g in got]}
    return out


def device_part(a):
    import torch
    import vocab_synth as VS
    from pyorbslam_amd import synth
    from pyorbslam_amd._lib import call
    from pyorbslam_amd.batch import KP_DTYPE, BatchView, StereoFrontEnd
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    t = VS.make_full_tree(seed=7, k=10, L=6)
    v = TemplatedVocabulary(k=10, L=6).from_arrays(t["parent"], t["is_leaf"], t["desc"], t["weight"])
    B = a.batch
    base = [synth.make_pair(100 + s) for s in range((B + 3) // 4)]
    imgs = np.stack([np.roll(im, -3 * (i % 4), axis=1) for i in range(B) for im in base[i // 4]])
    d_imgs = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    fe = StereoFrontEnd(imgs.shape[2], imgs.shape[1], max_pairs=B)
    s = torch.cuda.current_stream()
    fe.enqueue(d_imgs, stream_ptr=s.cuda_stream)
    fe.bow(v, levels_up=4, side="left", stream_ptr=s.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0.record(s)
        for _ in range(reps):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    pair_sets = {p: np.array([[i % B, (i + 1) % B] for i in range(p)], np.int32) for p in a.pairs}
    fe.match_bow(pair_sets[max(a.pairs)], nnratio=0.75, stream_ptr=s.cuda_stream)  # allocates for the largest set
    view = BatchView()
    call("orbfe_batch_view_get", fe.handle, C.byref(view))
    cap, mt = fe.kp_cap, fe._match

    def launch(p):
        call("orbfe_bow_match_device", C.c_void_p(view.desc), 2 * cap, C.c_void_p(view.count), 2, B,
             C.c_void_p(view.kps + KP_DTYPE.fields["angle"][1]), 6, None, 0, None, 0, C.byref(fe._bow["out"]), cap,
             C.c_void_p(mt["pairs"].data_ptr()), p, 50, 0, 0.75, C.byref(mt["out"]), cap, C.c_void_p(s.cuda_stream))

    res = {str(p): [] for p in a.pairs}
    bow = []
    for _ in range(a.rounds):
        for p in a.pairs:
            res[str(p)].append(timed(lambda p=p: launch(p), a.reps))
        bow.append(timed(lambda: fe.bow(v, levels_up=4, side="left", stream_ptr=s.cuda_stream), a.reps))
    torch.cuda.synchronize()
    n_raw = mt["n_raw"][:max(a.pairs)].cpu().numpy()
    counts = [len(fe.fetch_image(2 * i)[0]) for i in range(min(B, 4))]
    return {"batch_pairs": B, "features_first_frames": counts, "bow_ms": spread(bow), "status": fe.bow_status(),
            "match_kernel_ms": {p: spread(x) for p, x in res.items()},
            "raw_matches_per_pair_mean": round(float(n_raw.mean()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cands", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 64, 512])
    ap.add_argument("--feats", type=int, default=1500)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()  # before liborbfe's first device call: torch finds no device once another HIP user came first
    out = {"metric": "BoW-guided match, many pairs per launch (k_bow_match)", "rounds": a.rounds}
    if not a.device_only:
        out["kf_kf_many_vs_loop"] = host_part(a)
    out["device"] = device_part(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
