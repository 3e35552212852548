"""Time of training a vocabulary on the device (orbfe_vocab_train) on descriptors with a real distribution: those
the front-end extracts from the bench's synthetic stereo images (pyorbslam_amd.synth.make_batch, both images of a
pair as training images).

Two sizes: about 10^5 descriptors at k=10 L=3 and about 10^6 at k=10 L=5.  Per size: the call's wall time (upload of
the descriptors included; a host clock around the synchronous call), the stream time the call reports per depth (HIP
events: kernels and the small per-node read-backs between them), the Lloyd iterations, and
descriptors x iterations per second of stream time, with n_desc x (the sum over the depths of the depth's mean
iterations per node) as the work.  For scale only, the NumPy definition's time on the small size.

  python tools/bench_vocab_train.py [--small-pairs 26] [--large-pairs 250] [--reps 3] [--no-definition]
Writes profiles/vocab_train/bench_vocab_train.json.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def extract(n_pairs: int, chunk: int = 50) -> list:
    """Descriptors of both images of the synthetic pairs 0 .. n_pairs - 1, one array per image."""
    import torch
    from pyorbslam_amd import synth
    from pyorbslam_amd.batch import StereoFrontEnd
    fe = StereoFrontEnd(max_pairs=chunk)
    frames = []
    for p0 in range(0, n_pairs, chunk):
        n = min(chunk, n_pairs - p0)
        fe.enqueue(torch.from_numpy(synth.make_batch(n, seed0=p0)).cuda(), n)
        torch.cuda.synchronize()
        frames += [fe.fetch_image(i)[1] for i in range(2 * n)]
    return frames


def run(frames, k, L, reps):
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    out = []
    for _ in range(reps + 1):  # the first call warms up: code objects, allocations
        voc = TemplatedVocabulary(k, L)
        t0 = time.perf_counter()
        voc.create(frames, seed=0)
        wall = (time.perf_counter() - t0) * 1e3
        st = voc.train_stats()
        out.append((wall, st))
    out = out[1:]
    wall = sorted(w for w, _ in out)
    st = min((s for _, s in out), key=lambda s: s["kernel_ms"])
    depths = [d for d in range(L) if st["nodes_split"][d]]
    iters = [st["iter_sum"][d] / max(st["nodes_split"][d], 1) for d in depths]
    work = st["n_desc"] * sum(iters)
    return dict(k=k, L=L, n_images=len(frames), n_desc=st["n_desc"], n_nodes=st["n_nodes"], n_words=st["n_words"],
                reps=reps, wall_ms_min=wall[0], wall_ms_median=wall[len(wall) // 2], wall_ms_all=wall,
                stream_ms=st["kernel_ms"], stream_ms_all=[s["kernel_ms"] for _, s in out],
                depth_ms=[st["depth_ms"][d] for d in depths], weight_ms=st["weight_ms"],
                nodes_split=[st["nodes_split"][d] for d in depths], iter_sum=[st["iter_sum"][d] for d in depths],
                iter_max=[st["iter_max"][d] for d in depths], capped=[st["capped"][d] for d in depths],
                empty_dropped=[st["empty_dropped"][d] for d in depths], mean_iterations_per_depth=iters,
                desc_iterations_per_s=work / (st["kernel_ms"] * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-pairs", type=int, default=26)
    ap.add_argument("--large-pairs", type=int, default=250)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-definition", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vocab_train" / "bench_vocab_train.json"))
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_vocab_train needs a GPU"
    from pyorbslam_amd import _lib
    res = dict(device=torch.cuda.get_device_name(0), build_id=_lib.build_id(),
               data="descriptors of both images of pyorbslam_amd.synth.make_batch pairs (1241x376, 2000 features)")
    frames = extract(a.large_pairs)
    small = frames[:2 * a.small_pairs]
    res["small"] = run(small, 10, 3, a.reps)
    print(json.dumps(res["small"]), flush=True)
    res["large"] = run(frames, 10, 5, a.reps)
    print(json.dumps(res["large"]), flush=True)
    if not a.no_definition:
        import vocab_train_definition as VD
        t0 = time.perf_counter()
        t = VD.train(small, 10, 3)
        res["definition_small_s"] = time.perf_counter() - t0
        res["definition_small_nodes"] = int(len(t["parent"]))
        assert res["definition_small_nodes"] == res["small"]["n_nodes"]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))


if __name__ == "__main__":
    main()
