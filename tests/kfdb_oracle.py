"""CPU restatement of place recognition for the tests (and the baseline of tools/kfdb_bench.py).

Three pieces, all plain Python:
  l1_canonical        the canonical L1 score: terms (|vi - wi| - |vi|) - |wi| added in ascending word id,
                      sequentially, in double; -sum / 2.0 (GeneralScoring.l1_score sums the same terms in
                      CPython's set order, ScoringObject.py:8-28)
  query_arrays        what orbfe_kfdb_query returns for a list of stored vectors: common / first / score
  OracleKeyFrameDatabase
                      the reference's algorithm (KeyFrameDatabase.py): an inverted file word -> keyframes, the
                      walk over (query word x keyframes holding it), the word gate, the score gate, the
                      covisibility accumulation and the retain rule, scoring with l1_canonical
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
EPS = 2.0 ** -52


def score_bound(n_common: int) -> float:
    """|canonical - reference| for L1-normalised vectors: any two summation orders of the n_common terms differ
    by at most (n_common + 3) * 2^-52 after the division by 2; the tests allow one more."""
    return (n_common + 4) * EPS


def l1_canonical(v1, v2) -> float:
    s = 0.0
    for k in sorted(set(v1.keys()) & set(v2.keys())):
        vi = float(v1[k])
        wi = float(v2[k])
        s += (abs(vi - wi) - abs(vi)) - abs(wi)
    return -s / 2.0


def query_arrays(vectors, q):
    """vectors: one BoW dict per slot, None for an erased slot.  Returns int32 common, int32 first, f64 score."""
    n = len(vectors)
    common = np.zeros(n, np.int32)
    first = np.full(n, -1, np.int32)
    score = np.full(n, -0.0, np.float64)
    qk = set(q.keys())
    for s, v in enumerate(vectors):
        if v is None:
            continue
        sh = qk & set(v.keys())
        common[s] = len(sh)
        if sh:
            first[s] = min(sh)
        score[s] = l1_canonical(q, v)
    return common, first, score


class OracleVocabulary:
    """score() only: what KeyFrameDatabase needs of a vocabulary."""

    @staticmethod
    def score(v1, v2):
        return l1_canonical(v1, v2)


class OracleKeyFrameDatabase:
    def __init__(self, voc=None):
        self.voc = voc or OracleVocabulary()
        self.inv = {}

    def add(self, kf):
        for w in kf.mBowVec.keys():
            self.inv.setdefault(w, []).append(kf)

    def erase(self, kf):
        for w in kf.mBowVec.keys():
            lst = self.inv.get(w)
            if lst is not None and kf in lst:
                lst.remove(kf)

    def clear(self):
        self.inv = {}

    def detect_loop_candidates(self, q, min_score):
        connected = q.get_connected_key_frames()
        sharing = []
        for w in q.mBowVec.keys():
            for kf in self.inv.get(w, ()):
                if kf.mnLoopQuery != q.mnId:
                    kf.mnLoopWords = 0
                    if kf not in connected:
                        kf.mnLoopQuery = q.mnId
                        sharing.append(kf)
                kf.mnLoopWords += 1
        if not sharing:
            return []
        gate = int(max(kf.mnLoopWords for kf in sharing) * 0.8)
        scored = []
        for kf in sharing:
            if kf.mnLoopWords > gate:
                kf.mLoopScore = self.voc.score(q.mBowVec, kf.mBowVec)
                if kf.mLoopScore >= min_score:
                    scored.append((kf.mLoopScore, kf))
        if not scored:
            return []
        acc, best_acc = [], min_score
        for sc, kf in scored:
            a, b, bk = sc, sc, kf
            for k2 in kf.get_best_covisibility_key_frames(10):
                if k2.mnLoopQuery == q.mnId and k2.mnLoopWords > gate:
                    a += k2.mLoopScore
                    if k2.mLoopScore > b:
                        bk, b = k2, k2.mLoopScore
            acc.append((a, bk))
            if a > best_acc:
                best_acc = a
        keep = 0.75 * best_acc
        out, seen = [], set()
        for a, kf in acc:
            if a > keep and kf not in seen:
                out.append(kf)
                seen.add(kf)
        return out

    def detect_relocalization_candidates(self, f):
        sharing = []
        for w in f.mBowVec.keys():
            for kf in self.inv.get(w, ()):
                if kf.mnRelocQuery != f.mnId:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = f.mnId
                    sharing.append(kf)
                kf.mnRelocWords += 1
        if not sharing:
            return []
        gate = int(max(kf.mnRelocWords for kf in sharing) * 0.8)
        scored = []
        for kf in sharing:
            if kf.mnRelocWords > gate:
                kf.mRelocScore = self.voc.score(f.mBowVec, kf.mBowVec)
                scored.append((kf.mRelocScore, kf))
        if not scored:
            return []
        acc, best_acc = [], 0
        for sc, kf in scored:
            a, b, bk = sc, sc, kf
            for k2 in kf.get_best_covisibility_key_frames(10):
                if k2.mnRelocQuery != f.mnId:
                    continue
                a += k2.mRelocScore
                if k2.mRelocScore > b:
                    bk, b = k2, k2.mRelocScore
            acc.append((a, bk))
            best_acc = max(best_acc, a)
        keep = 0.75 * best_acc
        out, seen = [], set()
        for a, kf in acc:
            if a > keep and kf not in seen:
                out.append(kf)
                seen.add(kf)
        return out


# ---- stand-in keyframes and the recorded operation sequences (tests/golden/kfdb_<case>.npz) --------------------

OP_ADD, OP_ERASE, OP_LOOP, OP_RELOC = 0, 1, 2, 3
ATTRS = ("mnLoopQuery", "mnLoopWords", "mnRelocQuery", "mnRelocWords")


class StandInKF:
    """What KeyFrameDatabase reads and writes of a KeyFrame (query attributes as KeyFrame.__init__ sets them:
    no mLoopScore until a query assigns it)."""

    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = bow
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = 0.0
        self.connected = set()
        self.covis = []

    def get_connected_key_frames(self):
        return set(self.connected)

    def get_best_covisibility_key_frames(self, n):
        return self.covis[:n]


def world_from_golden(g):
    """Fresh stand-in keyframes of a golden: vectors, connected sets and ordered covisibility lists."""
    from collections import OrderedDict
    off = g["bow_off"]
    kfs = []
    for i in range(len(off) - 1):
        w = g["bow_word"][off[i]:off[i + 1]].tolist()
        v = g["bow_weight"][off[i]:off[i + 1]].tolist()
        kfs.append(StandInKF(int(g["kf_id"][i]), OrderedDict(zip(w, v))))
    for i, kf in enumerate(kfs):
        kf.connected = {kfs[j] for j in g["conn_idx"][g["conn_off"][i]:g["conn_off"][i + 1]].tolist()}
        kf.covis = [kfs[j] for j in g["covis_idx"][g["covis_off"][i]:g["covis_off"][i + 1]].tolist()]
    return kfs


def state_of(kfs):
    """(int attributes [n, 4], mLoopScore presence [n], mLoopScore [n], mRelocScore [n])"""
    ints = np.array([[getattr(k, a) for a in ATTRS] for k in kfs], np.int64)
    has = np.array([hasattr(k, "mLoopScore") for k in kfs], np.bool_)
    ls = np.array([getattr(k, "mLoopScore", 0.0) for k in kfs], np.float64)
    rs = np.array([k.mRelocScore for k in kfs], np.float64)
    return ints, has, ls, rs


def run_sequence(g, db, kfs, on_query):
    """Replay a golden's operation sequence on db; on_query(query number, returned keyframe indices) after each
    query.  ops rows: (op, keyframe index, min_score as f64 bits are in op_min)."""
    index = {id(k): i for i, k in enumerate(kfs)}
    qn = 0
    for (op, i), ms in zip(g["ops"].tolist(), g["op_min"].tolist()):
        kf = kfs[i]
        if op == OP_ADD:
            db.add(kf)
        elif op == OP_ERASE:
            db.erase(kf)
        else:
            got = db.detect_loop_candidates(kf, ms) if op == OP_LOOP else db.detect_relocalization_candidates(kf)
            on_query(qn, [index[id(k)] for k in got])
            qn += 1
    return qn


def n_common(kfs, a, b):
    return len(set(kfs[a].mBowVec) & set(kfs[b].mBowVec))


def load_golden(case):
    z = np.load(GOLDEN / f"kfdb_{case}.npz", allow_pickle=False)
    return {k: z[k] for k in z.files}


def check_against_golden(g, kfs, q, got):
    """State after query q against the reference's: exact ids / integers / presence, scores within the bound."""
    assert got == g["ret_idx"][g["ret_off"][q]:g["ret_off"][q + 1]].tolist(), f"query {q}: returned keyframes"
    ints, has, ls, rs = state_of(kfs)
    assert np.array_equal(ints, g["state_int"][q]), f"query {q}: integer attributes"
    assert np.array_equal(has, g["has_loop_score"][q]), f"query {q}: mLoopScore presence"
    for mine, ref, setter in ((ls, g["loop_score"][q], g["loop_setter"][q]),
                              (rs, g["reloc_score"][q], g["reloc_setter"][q])):
        for i in np.flatnonzero(mine != ref).tolist():
            assert setter[i] >= 0, f"query {q}: keyframe {i} has a score nobody set"
            bound = score_bound(n_common(kfs, int(setter[i]), i))
            assert abs(mine[i] - ref[i]) <= bound, (q, i, mine[i], ref[i], bound)
