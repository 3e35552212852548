"""Generate the golden of relocalisation's projection search: tests/golden/fkf.npz.

Imports the REFERENCE ORBMatcher.py read-only from the directory given on the command line (it imports only numpy)
and runs its own search_by_projection_f_kf_f of one frame against keyframes 0..5 of a tests/fuse_cases.py clone_world
of 7 keyframes with 300 features each and float32 poses; the frame has keyframe 6's features and its pose, moved a
little.  Four configurations: th / ORBdist of 10 / 100 and of 3 / 64, each with and without the orientation check;
every search starts from a frame of its own with the same pre-filled quarter of its slots, and has a non-empty
sAlreadyFound.  A few map points are mirrored through the frame's camera centre, so they project from behind.

Seeds are searched until some search finds at least 20 matches, some item's best feature was taken by an earlier item
of its search, the rotation histogram removes a match (with no tie at any histogram's cut) and a point behind the
camera reaches a cell window.  The array oracle with its redo (tests/fkf_oracle.py) must reproduce the reference on
every search of the stored world, every unmarked item deciding as the reference's loop body, with at most 2 % of the
items that reach a cell window marked; a file that breaks any of this is not written.  Stored: the world's arrays,
the frame's pose, the pre-fill, the found sets, and per configuration the six n and the frames' encoded slots.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_fkf.py <reference directory>
"""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import fkf_cases as KC  # noqa: E402
import fuse_cases as FC  # noqa: E402


def scene(RM, seed):
    z = KC.make_extras(FC.clone_world(seed), seed + 1)
    zz = FC.Z(z)
    stats, out = {}, dict(z)
    best = 0
    for cfg in range(len(KC.CONFIGS)):
        ref = KC.drive(zz, KC.loop_single(RM.ORBMatcher), cfg)
        mine = KC.drive(zz, KC.by_oracle(stats, agree=True), cfg)
        assert KC.same(mine, ref), "oracle against the reference"
        best = max(best, max(ref[0]))
        out[f"fkf_n{cfg}"], out[f"fkf_slots{cfg}"] = np.array(ref[0], np.int32), ref[1]
    share = stats["marginal"] / max(stats["reached"], 1)
    print("seed", seed, "most matches", best, stats, "marginal share %.4f" % share)
    if not (best >= 20 and stats["taken"] > 0 and stats["rotated"] > 0 and stats["behind"] > 0 and stats["stable"]
            and share <= 0.02):
        return None
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import ORBMatcher as RM  # noqa: E402
    warnings.simplefilter("ignore", DeprecationWarning)
    for seed in range(9100, 9500):
        out = scene(RM, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no world with the wanted events; not written")
    np.savez_compressed(HERE / "fkf.npz", **out)
    print("seed", seed, (HERE / "fkf.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
