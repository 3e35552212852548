"""Generate the golden of loop closing's mutual Sim3 search: tests/golden/sim3_many.npz.

Imports the REFERENCE ORBMatcher.py read-only from the directory given on the command line (it imports only numpy)
and runs its own search_by_sim3 from keyframe 0 to keyframes 1..6 of a tests/fuse_cases.py clone_world of 7 keyframes
with 300 features each and float32 poses, th = 7.5.  s12 is 1.0, 1.1 or 0.9; R12 and t12 come from the two poses as
tests/matcher_world.py's drive builds them, t12 moved by a small seeded perturbation so that the mutual check has
something to refuse; about a quarter of each vpMatches12 is pre-filled.

Seeds are searched until some pair finds at least 20 matches, some direction-1 winner is refused by the mutual check,
one pre-filled point has a valid index in its pKF2 and another has -1.  The array oracle with its redo of marked items
(tests/sim3_oracle.py) must reproduce the reference on every pair of the stored world, every unmarked item deciding
as the reference's loop body, with at most 2 % of the items that reach a cell window marked; a file that breaks any
of this is not written.  Stored: the world's arrays, the Sim3s, the pre-fills, and per pair n and the encoded
vpMatches12.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_sim3.py <reference directory>
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import fuse_cases as FC  # noqa: E402
import matcher_world as MW  # noqa: E402
import sim3_cases as SC  # noqa: E402
import sim3_oracle as S3  # noqa: E402


def scene(RM, seed):
    z = FC.clone_world(seed)
    z.update(SC.make_sim3s(MW.build(FC.Z(z)), seed + 1))
    zz = FC.Z(z)
    m = RM.ORBMatcher()
    n_pairs = FC.N_KF - 1
    w = MW.build(zz)
    ns, vms = SC.drive(w, zz, SC.loop_single(m.search_by_sim3), n_pairs)
    stats = {}
    w2 = MW.build(zz)
    mine = SC.drive(w2, zz, lambda kf1, kfs2, vs, ss, Rs, ts, th: S3.replay(
        kf1, list(zip(kfs2, vs, ss, Rs, ts)), th, stats=stats, agree=True), n_pairs)
    assert mine[0] == ns and all(np.array_equal(a, b) for a, b in zip(mine[1], vms)), "oracle against the reference"
    w3 = MW.build(zz)
    valid = minus = 0
    for kf2, vm, *_ in SC.pairs_of(w3, zz, n_pairs):
        idx = [p.get_index_in_keyframe(kf2) for p in vm if p]
        valid += sum(0 <= i < kf2.N for i in idx)
        minus += sum(i == -1 for i in idx)
    share = stats["marginal"] / max(stats["reached"], 1)
    print("seed", seed, "n", ns, stats, "pre-filled valid", valid, "minus", minus, "marginal share %.4f" % share)
    if not (max(ns) >= 20 and stats["refused"] > 0 and valid > 0 and minus > 0 and share <= 0.02):
        return None
    out = dict(z)
    for j, (n, vm) in enumerate(zip(ns, vms), 1):
        out[f"sim3_n{j}"], out[f"sim3_matches{j}"] = np.int32(n), vm
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import ORBMatcher as RM  # noqa: E402
    for seed in range(7500, 7600):
        out = scene(RM, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no world with the wanted events; not written")
    np.savez_compressed(HERE / "sim3_many.npz", **out)
    print("seed", seed, (HERE / "sim3_many.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
