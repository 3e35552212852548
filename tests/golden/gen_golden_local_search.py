"""Generate the golden of tracking's local-map search: tests/golden/local_search.npz.

Imports the REFERENCE Frame.py and ORBMatcher.py read-only from the directory given on the command line and runs the
loop of Tracking.search_local_points (Tracking.py:439-468) with the reference's own Frame.is_in_frustum and
ORBMatcher.search_by_projection_f_p, on Frame.__new__ instances that share the attributes of the stand-in frames of
tests/local_search_cases.py (so Frame.get_features_in_area is the reference's too), in a tests/fuse_cases.py
clone_world of 7 keyframes with 300 features each.  Two frames (the features of keyframes 5 and 6, their poses moved a
little) search the same local map of a few hundred points one after the other; some points were already seen in the
frame, some of those still carry a stale projection, some points are bad, and every frame has slots filled before the
call, by points with and without observations.  Six configurations: float64 and float32 poses and positions, th 1 and
5, nnratio 0.8 and 1.

Seeds are searched until every configuration assigns at least 20 points in some frame, some item is redone because a
feature of its was taken, a stale point is searched and the ratio test rejects a match.  The array oracle with its redo
(tests/local_search_oracle.py) must reproduce the reference on every configuration, with at most 5 % of the items
redone; a file that breaks any of this is not written.  Stored: the arrays of the two frames and of the map points,
what make_extras added, and per configuration the results and the snapshot of everything a call leaves behind.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_local_search.py <reference directory>
"""
from __future__ import annotations

import sys
import types
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import fuse_cases as FC  # noqa: E402
import local_search_cases as LC  # noqa: E402


def reference_run(RFrame, RM):
    """The loop with the reference's two methods, each on a reference Frame that shares the stand-in's attributes."""
    def twin(F):
        f = RFrame.Frame.__new__(RFrame.Frame)
        f.__dict__ = F.__dict__
        return f
    return LC.by_loop(lambda F, p, limit: twin(F).is_in_frustum(p, limit),
                      lambda F, vp, th, nn: RM.ORBMatcher(nn, True).search_by_projection_f_p(twin(F), vp, th))


def scene(RFrame, RM, seed):
    z = LC.make_extras(FC.clone_world(seed), seed + 1)
    zz = FC.Z(z)
    keep = [k for k in z if k.startswith(("kf5_", "kf6_", "mp_", "ls_"))]
    out = {k: z[k] for k in keep}
    stats = {}
    most = []
    for cfg in range(len(LC.CONFIGS)):
        ref = LC.drive(zz, reference_run(RFrame, RM), cfg)
        mine = LC.drive(zz, LC.by_oracle(stats), cfg)
        assert LC.same(mine, ref), ("oracle against the reference", cfg, LC.diff(mine, ref))
        most.append(int(ref[0][:, 1].max()))
        out[f"ls_res{cfg}"] = ref[0]
        for k, v in ref[1].items():
            out[f"ls_{k}{cfg}"] = v
    share = len(stats["redone"]) / max(stats["items"], 1)
    print("seed", seed, "most", most, {k: (len(v) if k == "redone" else v) for k, v in stats.items()},
          "redone share %.4f" % share)
    if not (min(most) >= 20 and stats["taken"] > 0 and stats["stale"] > 0 and stats["ratio"] > 0 and share < 0.05):
        return None
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, sys.argv[1])
    import Frame as RFrame  # noqa: E402
    import ORBMatcher as RM  # noqa: E402
    warnings.simplefilter("ignore")
    for seed in range(9600, 9700):
        out = scene(RFrame, RM, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no world with the wanted events; not written")
    np.savez_compressed(HERE / "local_search.npz", **out)
    print("seed", seed, (HERE / "local_search.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
