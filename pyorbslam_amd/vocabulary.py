"""Drop-in for pyDBoW.TemplatedVocabulary's loader and transform (pyDBoW/TemplatedVocabulary.py:23-160).

The reference descends the vocabulary tree one descriptor at a time in Python, with a per-byte popcount
per child (FORB.distance, FORB.py:30-32): ~10 us x k x L per feature, ~1 s per 2000-feature frame on
ORBvoc (k=10, L=6).  Here the text file is parsed natively (orbfe_vocab_load_text), the tree is laid
out child-run-contiguous in HBM, and every descriptor of a frame (or of many frames) descends in one
k_vocab_descend launch (pyorbslam_amd/csrc/orbfe_vocab.hip).  What is sequential in the reference — threading
the previous feature's node id through descents that stop above the node level, accumulating the BoW weights in
feature order, the total in word order — is done per frame by k_bow_assemble on the device (one workgroup per
frame, every float sum in the reference's order); the host only turns the arrays into the dicts.  A frame longer
than ORBFE_BOW_MAX_FRAME is assembled on the host (_assemble).

score / score_many (TemplatedVocabulary.py:99-106): "L1_NORM", the scoring System.py:38 builds the vocabulary
with, runs on the device (k_bow_score, pyorbslam_amd/csrc/orbfe_kfdb.hip) in the canonical summation order
(ascending word id; within (n_common + 3) * 2^-52 of l1_score's CPython-set order).  The five other scoring
strings are plain host restatements of ScoringObject.py, per pair.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import (ORBFE_BOW_MAX_FRAME, ORBFE_EFORMAT, ORBFE_EREJECT, VOCAB_TRAIN_DEPTH_COUNTERS, BowOut, VocabInfo,
                   VocabTrainParams, VocabTrainStats, call, check, lib, ptr)

# the header codes of DBoW2's WeightingType and ScoringType
WEIGHTING_CODES = {"TF_IDF": 0, "TF": 1, "IDF": 2, "BINARY": 3}
SCORING_CODES = {"L1_NORM": 0, "L2_NORM": 1, "CHI_SQUARE": 2, "KL": 3, "BHATTACHARYYA": 4, "DOT_PRODUCT": 5}


def _code(table, value, what):
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"unknown {what} {value!r}: one of {sorted(table)}")
        return table[value]
    return int(value)  # the header integer load_from_text_file leaves in place of the string


# ScoringObject.py:30-92, restated for the host (no device path)
def _l2_score(v1, v2):
    shared = set(v1.keys()) & set(v2.keys())
    dot = sum(v1[k] * v2[k] for k in shared)
    if dot >= 1.0:
        return 1.0
    return 1.0 - np.sqrt(1.0 - dot)


def _chi_square_score(v1, v2):
    score = 0.0
    for k in set(v1.keys()) & set(v2.keys()):
        vi, wi = v1[k], v2[k]
        if vi + wi != 0.0:
            score += (vi * wi) / (vi + wi)
    return score * 2.0


def _kl_score(v1, v2):
    log_eps = np.log(np.finfo(float).eps)
    score = 0.0
    for k in v1.keys():
        vi, wi = v1[k], v2.get(k, 0)
        if wi > 0 and vi > 0:
            score += vi * np.log(vi / wi)
        elif vi > 0:
            score += vi * (np.log(vi) - log_eps)
    return score


def _bhattacharyya_score(v1, v2):
    return sum(np.sqrt(v1[k] * v2[k]) for k in set(v1.keys()) & set(v2.keys()))


def _dot_product_score(v1, v2):
    return sum(v1[k] * v2[k] for k in set(v1.keys()) & set(v2.keys()))


_HOST_SCORING = {"L2_NORM": _l2_score, "CHI_SQUARE": _chi_square_score, "KL": _kl_score,
                 "BHATTACHARYYA": _bhattacharyya_score, "DOT_PRODUCT": _dot_product_score}


def l1_score_many(bv, others):
    """Canonical L1 score of bv against every vector of others: ONE orbfe_bow_score launch."""
    from .kfdb import bow_arrays
    others = list(others)
    if not others:
        return []
    qw, qv = bow_arrays(bv)
    parts = [bow_arrays(o) for o in others]
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(w) for w, _ in parts], out=off[1:])
    word = np.ascontiguousarray(np.concatenate([w for w, _ in parts]), np.int32)
    weight = np.ascontiguousarray(np.concatenate([v for _, v in parts]), np.float64)
    n = len(parts)
    common, first, score = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    call("orbfe_bow_score", ptr(qw), ptr(qv), len(qw), ptr(off), ptr(word), ptr(weight), n, ptr(common), ptr(first),
         ptr(score))
    return score.tolist()


def _l1_score(v1, v2):
    return l1_score_many(v1, [v2])[0]


class BowArrays(NamedTuple):
    """One frame's BowVector and FeatureVector as arrays (the device's CSR form)."""
    word: np.ndarray     # int32, distinct word ids, ascending
    weight: np.ndarray   # float64, their normalised weights
    node: np.ndarray     # int32, distinct node ids, ascending
    end: np.ndarray      # int32, exclusive end of each node's run in idx
    idx: np.ndarray      # int32, kept feature indices grouped by node, ascending within a run
    n_kept: int

    def dicts(self):
        """(BowVector, FeatureVector) as transform() returns them: OrderedDicts of Python ints and floats in
        ascending key order, ({}, {}) for a frame without kept features."""
        if self.n_kept == 0:
            return {}, {}
        idx, end = self.idx.tolist(), self.end.tolist()
        fv = OrderedDict((nd, idx[a:b]) for nd, a, b in zip(self.node.tolist(), [0] + end[:-1], end))
        return OrderedDict(zip(self.word.tolist(), self.weight.tolist())), fv


class TemplatedVocabulary:
    def __init__(self, k=10, L=5, weighting="TF_IDF", scoring="L1_NORM"):
        self.k = k
        self.L = L
        self.weighting = weighting
        self.scoring = scoring
        self._h = None
        # the scoring function is fixed here from the constructor string (create_scoring_object,
        # TemplatedVocabulary.py:83-94); load_from_text_file later overwrites self.scoring with the header
        # integer without changing it.  An unknown string leaves None: score() then raises TypeError.
        self.scoring_object = _l1_score if scoring == "L1_NORM" else _HOST_SCORING.get(scoring)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and _lib._lib is not None:
            _lib._lib.orbfe_vocab_destroy(h)

    # TemplatedVocabulary.py:43-81
    def load_from_text_file(self, filename) -> bool:
        with open(filename, "r") as f:  # same exception as the reference for a missing file
            header = f.readline().strip().split()
        # the reference assigns k and L before validating the header (TemplatedVocabulary.py:46-53)
        self.k, self.L = int(header[0]), int(header[1])
        h = C.c_void_p()
        rc = lib().orbfe_vocab_load_text(str(filename).encode(), C.byref(h))
        if rc == ORBFE_EREJECT:
            print("Vocabulary loading failure: Invalid parameters in file!")
            return False
        if rc == ORBFE_EFORMAT:
            raise ValueError(lib().orbfe_last_error().decode(errors="replace"))
        check("orbfe_vocab_load_text", rc)
        self._replace(h)
        info = self.info()
        self.scoring, self.weighting = info.scoring, info.weighting
        return True

    def from_arrays(self, parent, is_leaf, desc, weight):
        """Install a tree given as per-node arrays (node 0 = root), e.g. one built in memory."""
        parent = np.ascontiguousarray(parent, np.int32)
        n = len(parent)
        leaf = np.ascontiguousarray(is_leaf, np.uint8)
        d = np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        w = np.ascontiguousarray(weight, np.float64)
        h = C.c_void_p()
        call("orbfe_vocab_create", int(self.k), int(self.L), 0, 0, n, ptr(parent), ptr(leaf), ptr(d), ptr(w),
             C.byref(h))
        self._replace(h)
        return self

    def create(self, training_features, seed=0, max_iter=64):
        """DBoW2's create: train the tree on the device (orbfe_vocab_train) from one (n_i, 32) uint8 array per image.
        k, L, weighting and scoring are the constructor's.  Returns self."""
        frames = [np.ascontiguousarray(f, np.uint8).reshape(-1, 32) for f in training_features]
        count = np.array([len(f) for f in frames], np.int32)
        start = np.zeros(len(frames), np.int64)
        np.cumsum(count[:-1], out=start[1:])
        d = np.ascontiguousarray(np.concatenate(frames)) if frames else np.zeros((0, 32), np.uint8)
        return self.train_arrays(d.ctypes.data if len(d) else None, False, start, count, seed, max_iter)

    def train_arrays(self, desc_ptr, on_device, start, count, seed=0, max_iter=64):
        """orbfe_vocab_train over image f = descriptors start[f] .. start[f] + count[f] of the host or device memory
        at desc_ptr, which the caller keeps alive during the call.  Returns self."""
        prm = VocabTrainParams(int(self.k), int(self.L), _code(WEIGHTING_CODES, self.weighting, "weighting"),
                               _code(SCORING_CODES, self.scoring, "scoring"), int(max_iter), 0,
                               int(seed) & 0xFFFFFFFFFFFFFFFF)
        start = np.ascontiguousarray(start, np.int64)
        count = np.ascontiguousarray(count, np.int32)
        h, st = C.c_void_p(), VocabTrainStats()
        call("orbfe_vocab_train", C.c_void_p(desc_ptr), 1 if on_device else 0, ptr(start), ptr(count), len(count),
             C.byref(prm), C.byref(h), C.byref(st))
        self._replace(h)
        self._train_stats = st
        return self

    def train_stats(self) -> dict:
        """Counters and times of the create() that built this vocabulary (orbfe_vocab_train_stats); the per-depth
        lists have one entry per depth 0 .. 9 of the nodes that were split."""
        st = getattr(self, "_train_stats", None)
        if st is None:
            raise RuntimeError("this vocabulary was not trained by create()")
        out = dict(n_desc=int(st.n_desc), n_nodes=int(st.n_nodes), n_words=int(st.n_words),
                   weight_ms=float(st.weight_ms), kernel_ms=float(st.kernel_ms), depth_ms=list(st.depth_ms))
        for key in VOCAB_TRAIN_DEPTH_COUNTERS:
            out[key] = list(getattr(st, key))
        return out

    def save_to_text_file(self, filename) -> None:
        """The text layout load_from_text_file (here and in the reference) reads (orbfe_vocab_save_text)."""
        call("orbfe_vocab_save_text", self._handle(), str(filename).encode())

    def _replace(self, h):
        old, self._h = self._h, h
        self._train_stats = None  # train_arrays sets them after installing its tree
        if old is not None:
            lib().orbfe_vocab_destroy(old)

    def _handle(self):
        if self._h is None:  # an unloaded vocabulary is the bare root (TemplatedVocabulary.py:36)
            h = C.c_void_p()
            call("orbfe_vocab_create", int(self.k), int(self.L), 0, 0, 1, None, None, None, None, C.byref(h))
            self._h = h
        return self._h

    def info(self) -> VocabInfo:
        out = VocabInfo()
        call("orbfe_vocab_get_info", self._handle(), C.byref(out))
        return out

    def node_arrays(self) -> dict:
        n = int(self.info().n_nodes)
        a = dict(parent=np.zeros(n, np.int32), is_leaf=np.zeros(n, np.uint8), desc=np.zeros((n, 32), np.uint8),
                 weight=np.zeros(n, np.float64), word_id=np.zeros(n, np.int32))
        call("orbfe_vocab_get_nodes", self._handle(), *(ptr(a[k]) for k in ("parent", "is_leaf", "desc", "weight",
                                                                            "word_id")))
        return a

    # TemplatedVocabulary.py:96-97
    def size(self) -> int:
        return 0 if self._h is None else int(self.info().n_words)

    # TemplatedVocabulary.py:99-106
    def score(self, bow_vector1, bow_vector2):
        return self.scoring_object(bow_vector1, bow_vector2)

    def score_many(self, bow_vector, bow_vectors):
        """[score(bow_vector, b) for b in bow_vectors]; under L1_NORM one kernel launch for all of them."""
        if self.scoring_object is _l1_score:
            return l1_score_many(bow_vector, bow_vectors)
        return [self.scoring_object(bow_vector, b) for b in bow_vectors]

    def descend(self, features, levels_up=4):
        """Raw per-descriptor (word id, node id at depth L - levels_up or -1, weight): one launch."""
        q = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
        n = len(q)
        word = np.zeros(n, np.int32)
        node = np.zeros(n, np.int32)
        w = np.zeros(n, np.float64)
        if n:
            call("orbfe_vocab_transform", self._handle(), ptr(q), n, int(self.L - levels_up), ptr(word), ptr(node),
                 ptr(w))
        return word, node, w

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        call("orbfe_vocab_last_ms", self._handle(), C.byref(ms))
        return float(ms.value)

    @staticmethod
    def _assemble(word, node, w):
        """BowVector + FeatureVector of one frame from its raw descents (TemplatedVocabulary.py:108-129;
        BowVector.py:8-35; FeatureVector.py:8-17)."""
        n = len(word)
        if n == 0:
            return {}, {}
        # a descent that stops above the node level keeps the previous feature's node id (initially 0)
        src = np.maximum.accumulate(np.where(node >= 0, np.arange(n), -1))
        nid = np.where(src >= 0, node[np.maximum(src, 0)], 0)
        keep = np.flatnonzero(w > 0)
        if len(keep) == 0:
            return {}, {}
        acc: dict = {}
        feats: dict = {}
        for i, wid, nd, wt in zip(keep.tolist(), word[keep].tolist(), nid[keep].tolist(), w[keep].tolist()):
            acc[wid] = acc[wid] + wt if wid in acc else wt
            feats.setdefault(nd, []).append(i)
        bv = OrderedDict(sorted(acc.items()))
        total = sum(bv.values())
        if total > 0:
            for key in bv:
                bv[key] /= total
        return bv, OrderedDict(sorted(feats.items()))

    def bow_many(self, frames, levels_up=4):
        """BowArrays of every frame: the descent and k_bow_assemble (one workgroup per frame) in one
        orbfe_vocab_bow call, no per-feature host work.  word / weight are what BowDatabase.add_arrays and
        query_arrays take.  Raises OrbfeError (EINVAL) for a frame longer than ORBFE_BOW_MAX_FRAME."""
        frames = [np.ascontiguousarray(f, np.uint8).reshape(-1, 32) for f in frames]
        nf = len(frames)
        if nf == 0:
            return []
        off = np.zeros(nf + 1, np.int64)
        np.cumsum([len(f) for f in frames], out=off[1:])
        n = int(off[-1])
        q = np.ascontiguousarray(np.concatenate(frames))
        ints = np.zeros((4, max(n, 1)), np.int32)   # bow_word, fv_node, fv_end, fv_idx
        per = np.zeros((3, nf), np.int32)           # n_words, n_nodes, n_kept
        weight = np.zeros(max(n, 1), np.float64)
        out = BowOut(n_words=ptr(per[0]), bow_word=ptr(ints[0]), bow_weight=ptr(weight), n_nodes=ptr(per[1]),
                     fv_node=ptr(ints[1]), fv_end=ptr(ints[2]), fv_idx=ptr(ints[3]), n_kept=ptr(per[2]), status=None)
        call("orbfe_vocab_bow", self._handle(), ptr(q), ptr(off), nf, int(self.L - levels_up), C.byref(out))
        res = []
        for f, o in enumerate(off[:-1].tolist()):
            nw, nn, nk = per[:, f].tolist()
            res.append(BowArrays(ints[0, o:o + nw], weight[o:o + nw], ints[1, o:o + nn], ints[2, o:o + nn],
                                 ints[3, o:o + nk], nk))
        return res

    def last_bow_ms(self) -> float:
        """Kernel time (descent + assembly) of the last bow_many on this vocabulary."""
        ms = C.c_float()
        call("orbfe_vocab_bow_last_ms", self._handle(), C.byref(ms))
        return float(ms.value)

    # TemplatedVocabulary.py:108-129
    def transform(self, features, levels_up=4):
        return self.transform_many([features], levels_up)[0]

    def transform_many(self, frames, levels_up=4):
        """transform() of several frames with ONE descent launch and ONE assembly launch over all of them.  A frame
        longer than ORBFE_BOW_MAX_FRAME is descended on the device and assembled on the host (_assemble)."""
        frames = [np.ascontiguousarray(f, np.uint8).reshape(-1, 32) for f in frames]
        short = [i for i, f in enumerate(frames) if len(f) <= ORBFE_BOW_MAX_FRAME]
        out = [None] * len(frames)
        for i, a in zip(short, self.bow_many([frames[i] for i in short], levels_up)):
            out[i] = a.dicts()
        for i, f in enumerate(frames):
            if out[i] is None:
                out[i] = self._assemble(*self.descend(f, levels_up))
        return out

    # TemplatedVocabulary.py:131-160
    def transform_feature(self, feature, nid, levels_up):
        word, node, w = self.descend(np.asarray(feature).reshape(1, 32), levels_up)
        if nid is not None and node[0] >= 0:
            nid = int(node[0])
        return int(word[0]), nid, float(w[0])
