"""ABI 8's additions (orbfe_vocab_bow, orbfe_vocab_bow_device) on a GPU-less host: the symbols, the constants and the argument
checks that come before any device call."""
import ctypes as C
import re

import numpy as np

from conftest import ROOT


def test_abi_version_is_9():
    """9 = 8 (the entry points below) + orbfe_get_stereo_bucket_kernel, additive."""
    from pyorbslam_amd import _lib
    assert _lib.lib().orbfe_abi_version() == 9 == _lib.ORBFE_ABI_VERSION
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    assert int(re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1)) == 9


def test_new_symbols_resolve():
    from pyorbslam_amd import _lib
    L = _lib.lib()
    for name in ("orbfe_vocab_bow", "orbfe_vocab_bow_device", "orbfe_vocab_bow_scratch_bytes",
                 "orbfe_vocab_bow_last_ms"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert C.sizeof(_lib.BowOut) == 9 * C.sizeof(C.c_void_p)


def test_max_frame():
    from pyorbslam_amd import _lib
    hdr = (ROOT / "include" / "orbfe.h").read_text()
    n = int(re.search(r"#define ORBFE_BOW_MAX_FRAME (\d+)", hdr).group(1))
    assert n >= 8192 and n == _lib.ORBFE_BOW_MAX_FRAME


def test_null_vocabulary_is_refused_without_a_device():
    from pyorbslam_amd import _lib
    L = _lib.lib()
    out = _lib.BowOut()
    assert L.orbfe_vocab_bow(None, None, None, 0, 2, C.byref(out)) == _lib.ORBFE_EINVAL
    assert L.orbfe_vocab_bow_device(None, None, 0, None, 1, 0, 2, 0, C.byref(out), None, 0, None) == _lib.ORBFE_EINVAL
    ms = C.c_float()
    assert L.orbfe_vocab_bow_last_ms(None, C.byref(ms)) == _lib.ORBFE_EINVAL


def test_host_checks_that_need_no_device():
    """Zero frames, frames without descriptors, a frame above the limit and bad offsets never reach the device."""
    from pyorbslam_amd import _lib
    from pyorbslam_amd.vocabulary import TemplatedVocabulary
    L = _lib.lib()
    v = TemplatedVocabulary(k=3, L=2)
    h = v._handle()
    out = _lib.BowOut()
    assert L.orbfe_vocab_bow(h, None, None, 0, 1, C.byref(out)) == 0
    assert v.bow_many([]) == []
    got = v.bow_many([np.zeros((0, 32), np.uint8)] * 3)
    assert [(len(a.word), len(a.node), len(a.idx), a.n_kept) for a in got] == [(0, 0, 0, 0)] * 3
    assert v.transform(np.zeros((0, 32), np.uint8)) == ({}, {})
    per = np.full((3, 2), -7, np.int32)
    out = _lib.BowOut(n_words=_lib.ptr(per[0]), n_nodes=_lib.ptr(per[1]), n_kept=_lib.ptr(per[2]))
    for off in ([0, _lib.ORBFE_BOW_MAX_FRAME + 1, _lib.ORBFE_BOW_MAX_FRAME + 1], [1, 1, 1], [0, 5, 3]):
        o = np.array(off, np.int64)
        assert L.orbfe_vocab_bow(h, None, _lib.ptr(o), 2, 1, C.byref(out)) == _lib.ORBFE_EINVAL
        assert bool((per == -7).all())
    o = np.array([0, _lib.ORBFE_BOW_MAX_FRAME + 1], np.int64)
    assert L.orbfe_vocab_bow(h, None, _lib.ptr(o), 1, 1, C.byref(out)) == _lib.ORBFE_EINVAL
    msg = L.orbfe_last_error().decode()
    assert f"limit of {_lib.ORBFE_BOW_MAX_FRAME} per frame" in msg and str(_lib.ORBFE_BOW_MAX_FRAME + 1) in msg
    n = C.c_int64()
    assert L.orbfe_vocab_bow_scratch_bytes(64, 4056, C.byref(n)) == 0 and n.value == 64 * 4056 * 16
    assert L.orbfe_vocab_bow_scratch_bytes(-1, 4056, C.byref(n)) == _lib.ORBFE_EINVAL
