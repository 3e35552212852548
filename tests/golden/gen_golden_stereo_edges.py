"""Generate the reference goldens of the stereo matcher's boundary cases (build container only).

For every case of tests/stereo_cases.py the REFERENCE's Frame.compute_stereo_matches is called (through
gen_golden.import_reference / reference_stereo, which take bf and fx) on the oracle's extraction of the pair; the
restatement (oracle/stereo_oracle.py) must agree bit for bit.  One file per pair and extractor configuration,
tests/golden/stereo_edges_<group>.npz, holds for every fx the outputs (status, u_right, depth), once the four
input digests, and in `meta` the census of every fx as JSON.  Outputs and digests only: nothing of the
reference's text is stored.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_stereo_edges.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import gen_golden as G  # noqa: E402  (puts the repository root on sys.path)
import stereo_cases as SC  # noqa: E402
from oracle import stereo_oracle  # noqa: E402


def main():
    RFrame, _ = G.import_reference()
    for group in SC.GROUPS:
        left, right = SC.image_ref(group, 0), SC.image_ref(group, 1)
        arrays, censuses = {}, {}
        for case in SC.cases_of(group):
            u, d = G.reference_stereo(RFrame, left.kps, left.desc, right.kps, right.desc, left.sheared, right.sheared,
                                      left.tables, bf=case.bf, fx=case.fx)
            st, vu = stereo_oracle.encode(u)
            st_d, vd = stereo_oracle.encode(d)
            assert (st == st_d).all(), case.id
            rs, ru, rd, _ = SC.restate(left, right, case.bf, case.fx)
            assert (rs == st).all() and (ru == vu).all() and (rd == vd).all(), case.id
            counts, labels = SC.census(left, right, case.bf, case.fx)
            assert [SC.STATUS_OF_LABEL.get(x, 0) for x in labels] == st.tolist(), case.id
            arrays[f"{case.key}_status"], arrays[f"{case.key}_u_right"], arrays[f"{case.key}_depth"] = st, vu, vd
            censuses[case.key] = counts
            print(f"{case.id}: N={len(left.kps)} Nr={len(right.kps)} matched={int((st == 1).sum())} "
                  f"zero-disp={int((st == 2).sum())}")
        c0 = SC.cases_of(group)[0]
        meta = dict(pair=c0.pair, seed=SC.SEED, h=SC.H, w=SC.W, params=c0.params, bf=c0.bf, census=censuses)
        np.savez_compressed(G.GOLD / f"stereo_edges_{group}.npz", **arrays,
                            kps_left_sha=np.array(G.sha(left.kps)), desc_left_sha=np.array(G.sha(left.desc)),
                            kps_right_sha=np.array(G.sha(right.kps)), desc_right_sha=np.array(G.sha(right.desc)),
                            left_sha=np.array(G.sha(left.image)), right_sha=np.array(G.sha(right.image)),
                            meta=np.array(json.dumps(meta, sort_keys=True)))


if __name__ == "__main__":
    main()
