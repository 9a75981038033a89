"""The kvx_admm_batch_* entry points are declared, exported and bound, and answer with a status code -- not a crash -- on a
handle that was planned (host only) and never set up."""
import ctypes
import os
import re

import numpy as np

from kvxopt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["kvx_admm_batch_begin", "kvx_admm_batch_iterate", "kvx_admm_batch_state", "kvx_admm_batch_solution", "kvx_admm_batch_end"]


def test_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "kvxhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kvx_admm_batch_[a-z0-9_]+)\s*\(", src))
    assert declared == set(ENTRIES)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), "missing export: " + name
        assert name in _lib.exported_symbols()


def planned():
    """min x0 + x1  s.t.  0 <= x <= 1: a plan on the host."""
    L = _lib.lib()
    Ap, Ai, Ax = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int64), np.ones(2)
    q, l, u = np.ones(2), np.zeros(2), np.ones(2)
    h = _lib.vp()
    rc = L.kvx_admm_plan(2, 2, _lib.pi(Ap), _lib.pi(Ai), _lib.pd(Ax), None, None, None, _lib.pd(q), _lib.pd(l), _lib.pd(u), 10, None, None,
                         None, None, ctypes.byref(h))
    assert rc == _lib.KVX_OK
    return h


def test_entries_on_a_handle_that_is_not_set_up():
    L = _lib.lib()
    h = planned()
    try:
        Q, lo, up = np.ones((2, 3), order="F"), np.zeros((2, 3), order="F"), np.ones((2, 3), order="F")
        refused = (_lib.KVX_EINVAL, _lib.KVX_EDEVICE)
        assert L.kvx_admm_batch_begin(h, 3, _lib.pd(Q), _lib.pd(lo), _lib.pd(up)) in refused
        assert L.kvx_admm_batch_begin(h, 3, _lib.pd(Q), None, None) in refused
        out, run = np.zeros((3, 24)), np.ones(3, dtype=np.int64)
        assert L.kvx_admm_batch_iterate(h, 1, _lib.pi(run), _lib.pd(out)) in refused
        assert L.kvx_admm_batch_state(h, None, None, None, None, None) in refused
        X, Y = np.zeros((2, 3), order="F"), np.zeros((2, 3), order="F")
        assert L.kvx_admm_batch_solution(h, _lib.pi(np.zeros(3, dtype=np.int64)), _lib.pd(X), _lib.pd(Y)) in refused
        assert L.kvx_admm_batch_end(h) == _lib.KVX_OK                  # nothing to free
        # arguments that no handle accepts, with or without a device
        assert L.kvx_admm_batch_begin(None, 3, _lib.pd(Q), None, None) == _lib.KVX_EINVAL
        assert L.kvx_admm_batch_begin(h, 0, _lib.pd(Q), None, None) == _lib.KVX_EINVAL
        up[1, 2] = -1.0                                                  # l > u in member 2, row 1: refused on the host
        assert L.kvx_admm_batch_begin(h, 3, _lib.pd(Q), _lib.pd(lo), _lib.pd(up)) == _lib.KVX_EINVAL
        assert b"member 2, row 1" in L.kvx_last_error()
        up[1, 2] = 0.0                                                   # an equality where the kept row is two-sided
        assert L.kvx_admm_batch_begin(h, 3, _lib.pd(Q), _lib.pd(lo), _lib.pd(up)) == _lib.KVX_EINVAL
        assert b"member 2, row 1" in L.kvx_last_error()
        assert L.kvx_admm_batch_iterate(None, 1, _lib.pi(run), _lib.pd(out)) == _lib.KVX_EINVAL
        assert L.kvx_admm_batch_end(None) == _lib.KVX_EINVAL
    finally:
        L.kvx_admm_free(h)
