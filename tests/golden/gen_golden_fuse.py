"""Generate the golden of the many-keyframe fusion: tests/golden/fuse_many.npz.

Imports the REFERENCE ORBMatcher.py read-only from the directory given on the command line (it imports only numpy)
and runs its own fuse_pkf_mp the way LocalMapping.search_in_neighbors does (LocalMapping.py:357-375) on a
tests/matcher_world.py world of 7 keyframes with 300 features each: keyframe 0's get_map_point_matches() into
keyframes 1..n, th = 3.0, then the neighbours' pooled map points into keyframe 0, for n = 1, 3 and 6 on fresh
builds.  make_world alone gives no replace in these loops (every re-observed feature's slot is empty or holds the
same point), so a share of the map points is cloned at nearly the same position with a noisy descriptor and a share
of the neighbours' slots holds the clone instead.  Seeds are searched until the run with 6 neighbours has at least
20 replace events in both directions, a point skipped in a later keyframe because an earlier replace of the call
made it bad, and an item replayed after its point's descriptor changed; the array oracle with its replay
(tests/fuse_oracle.py) must reproduce the reference's results on the stored world, with at most 2 % of the items
that reach a cell window marked marginal.  Stored: the world's arrays, and per n the return values, the event log,
the final slots, the bad flags and the descriptors.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_fuse.py <reference directory>
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import fuse_cases as FC  # noqa: E402
import matcher_world as MW  # noqa: E402

def scene(RM, seed):
    z = FC.clone_world(seed)
    zz = FC.Z(z)
    m = RM.ORBMatcher()
    ref = lambda kfs, pts, th: [m.fuse_pkf_mp(kf, pts, th) for kf in kfs]  # noqa: E731
    out = dict(z)
    for n in FC.N_NEIGH:
        w = MW.build(zz)
        state = FC.world_state(w, FC.drive(w, ref, n))
        stats = {}
        w2 = MW.build(zz)
        mine = FC.world_state(w2, FC.drive(w2, FC.oracle_fuse(stats), n))
        FC.assert_state(mine, state, f"oracle against the reference, n = {n}")
        out.update({f"n{n}_{k}": v for k, v in state.items()})
    n_replace = int((state["log"][:, 0] == MW.EV_REPLACE).sum())
    share = stats["marginal"] / max(stats["reached"], 1)
    print("seed", seed, "replace", n_replace, stats, "marginal share %.4f" % share)
    ok = (n_replace >= 20 and stats["list_replaced"] > 0 and stats["slot_replaced"] > 0 and stats["became_bad"] > 0
          and stats["changed"] > 0 and share <= 0.02)
    return out if ok else None


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import ORBMatcher as RM  # noqa: E402
    for seed in range(7100, 7200):
        out = scene(RM, seed)
        if out is not None:
            break
    else:
        raise SystemExit("no world with the wanted events; not written")
    np.savez_compressed(HERE / "fuse_many.npz", **out)
    print("seed", seed, (HERE / "fuse_many.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
