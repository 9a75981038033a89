"""The C-ABI additions behind `kvxopt_amd.umfpack`: kvx_lu_analyze_opts (per-analysis flags) and kvx_lu_solve_refine / _dev are
declared in include/kvxhip.h with 64-bit integers, exported by the library, bound by _lib, and answer bad arguments with status
codes on any box."""
import ctypes
import os
import re

import numpy as np

from kvxopt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kvx_lu_analyze_opts", "kvx_lu_solve_refine", "kvx_lu_solve_refine_dev")


def header():
    return open(os.path.join(ROOT, "include", "kvxhip.h")).read()


def prototype(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header())
    assert m, "not declared: " + name
    return " ".join(m.group(1).split())


def test_new_symbols_are_declared_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        prototype(name)
        assert hasattr(L, name), "missing export: " + name
        assert name in _lib.exported_symbols()
    h = header()
    assert re.search(r"#define\s+KVX_LU_FLAG_NO_BTF\s+1\b", h) and _lib.KVX_LU_FLAG_NO_BTF == 1
    assert re.search(r"#define\s+KVX_LU_FLAG_KEEP_VALUES\s+2\b", h) and _lib.KVX_LU_FLAG_KEEP_VALUES == 2
    assert "umfpack.c:240-290" in h and "umfpack_*_symbolic" in h                 # what the new analysis entry replaces


def test_the_abi_is_64_bit():
    p = prototype("kvx_lu_analyze_opts")
    assert p == ("int64_t n, const int64_t *colptr, const int64_t *rowind, const double *values, int64_t flags, kvx_lu_sym **out")
    for name, buf in (("kvx_lu_solve_refine", "double *B"), ("kvx_lu_solve_refine_dev", "double *B_dev")):
        assert prototype(name) == "kvx_lu_num *N, int trans, %s, int64_t nrhs, int64_t ldB, int64_t steps, double *berr_out" % buf
    assert not re.search(r"\b(int|long|int32_t)\s+(n|nrhs|ldB|steps|flags)\b", " ".join(prototype(n) for n in NEW))
    i64 = ctypes.c_int64
    assert _lib._SIGS["kvx_lu_analyze_opts"][1][0] is i64 and _lib._SIGS["kvx_lu_analyze_opts"][1][4] is i64
    assert _lib._SIGS["kvx_lu_solve_refine"][1][3:6] == [i64, i64, i64]
    assert _lib._SIGS["kvx_lu_solve_refine_dev"][1][3:6] == [i64, i64, i64]


def test_flags_and_argument_checks_need_no_gpu():
    L = _lib.lib()
    vp = _lib.vp
    cp = np.array([0, 1, 2], dtype=np.int64); ri = np.array([0, 1], dtype=np.int64); v = np.array([1.0, 2.0])
    nb, nl = ctypes.c_int64(), ctypes.c_int64()
    blk = np.full(2, -1, dtype=np.int64)
    h = vp()
    assert L.kvx_lu_analyze_opts(2, _lib.pi(cp), _lib.pi(ri), _lib.pd(v), 4, ctypes.byref(h)) == _lib.KVX_EINVAL      # unknown flag bit
    assert L.kvx_lu_analyze_opts(0, _lib.pi(cp), _lib.pi(ri), _lib.pd(v), 1, ctypes.byref(h)) == _lib.KVX_EINVAL      # n < 1
    assert L.kvx_lu_analyze_opts(2, _lib.pi(cp), _lib.pi(ri), _lib.pd(v), 1, None) == _lib.KVX_EINVAL
    # a diagonal matrix is two blocks (tests/test_abi.py) -- one with the flag, two again afterwards
    for flags, want in ((0, 2), (_lib.KVX_LU_FLAG_NO_BTF, 1), (_lib.KVX_LU_FLAG_NO_BTF | _lib.KVX_LU_FLAG_KEEP_VALUES, 1), (0, 2)):
        assert L.kvx_lu_analyze_opts(2, _lib.pi(cp), _lib.pi(ri), _lib.pd(v), flags, ctypes.byref(h)) == _lib.KVX_OK
        assert L.kvx_lu_sym_btf(h, ctypes.byref(nb), ctypes.byref(nl), _lib.pi(blk)) == _lib.KVX_OK
        assert (nb.value, nl.value) == (want, 1) and sorted(blk) == list(range(want)) * (2 // want)
        L.kvx_lu_free_symbolic(h)
    assert L.kvx_lu_analyze(2, _lib.pi(cp), _lib.pi(ri), _lib.pd(v), ctypes.byref(h)) == _lib.KVX_OK                   # the old entry: flags 0
    assert L.kvx_lu_sym_btf(h, ctypes.byref(nb), ctypes.byref(nl), None) == _lib.KVX_OK and nb.value == 2
    L.kvx_lu_free_symbolic(h)
    w = np.zeros(2)
    for steps, berr in ((0, None), (2, None), (2, _lib.pd(w))):
        assert L.kvx_lu_solve_refine(None, 0, _lib.pd(v), 1, 2, steps, berr) == _lib.KVX_EINVAL
        assert L.kvx_lu_solve_refine_dev(None, 0, None, 1, 2, steps, berr) == _lib.KVX_EINVAL
