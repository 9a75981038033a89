"""Host-side checks of the nonlinear convex drivers (kvxopt_amd.cvx, solvers.gp / cp / cpl): the public names, the reference's
argument errors (cvxprog.py:2056-2092), the forms this restatement refuses, the plan of the log-sum-exp blocks (kvx_gp_plan)
against a numpy restatement of its two patterns, and the G23 / G24 fixtures.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

from kvxopt_amd import _lib, base, cvx, solvers

from gp_eval_numpy import assert_plan_patterns

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G23 = np.load(os.path.join(_GOLD, "g23_gp_eval.npz"))
G23_CASES = [str(c) for c in G23["cases"]]


def g23_ccs(name):
    """(K, n, Fp, Fi, Fx) of a G23 case: the sparse case by its nonzeros, the others with every entry."""
    F = G23[name + "__F"]
    if bool(G23[name + "__sparse"]):
        I, J = np.nonzero(F)
        F = base.spmatrix(F[I, J], I, J, F.shape)
    _, n, Fp, Fi, Fx = base.ccs(F)
    return G23[name + "__K"], n, Fp, Fi, Fx


def test_public_names_exist():
    for name in ("gp", "cp", "cpl"):
        assert callable(getattr(solvers, name))
    for line in ("cvxprog.py:35", "cvxprog.py:1359", "cvxprog.py:1967"):
        assert line in solvers.__doc__


def test_gp_argument_errors_are_the_references():
    F, g = base.matrix(np.ones((3, 2))), base.matrix(np.zeros(3))
    bad = [(dict(K=(1, 2), F=F, g=g), "'K' must be a list of positive integers"),
           (dict(K=[1, 0, 2], F=F, g=g), "'K' must be a list of positive integers"),
           (dict(K=[1.0, 2], F=F, g=g), "'K' must be a list of positive integers"),
           (dict(K=[2, 2], F=F, g=g), "'F' must be a dense or sparse 'd' matrix with 4 rows"),
           (dict(K=[1, 2], F=[[1.0]], g=g), "'F' must be a dense or sparse 'd' matrix with 3 rows"),
           (dict(K=[1, 2], F=F, g=base.matrix(np.zeros(2))), "'g' must be a dene 'd' matrix of size (3,1)"),
           (dict(K=[1, 2], F=F, g=base.spmatrix([1.0], [0], [0], (3, 1))), "'g' must be a dene 'd' matrix of size (3,1)"),
           (dict(K=[1, 2], F=F, g=g, G=base.matrix(np.ones((2, 3))), h=base.matrix(np.ones(2))),
            "'G' must be a dense or sparse 'd' matrix with 2 columns"),
           (dict(K=[1, 2], F=F, g=g, G=base.matrix(np.ones((2, 2))), h=base.matrix(np.ones(3))),
            "'h' must be a dense 'd' matrix of size (2,1)"),
           (dict(K=[1, 2], F=F, g=g, A=base.matrix(np.ones((1, 3))), b=base.matrix(np.ones(1))),
            "'A' must be a dense or sparse 'd' matrix with 2 columns"),
           (dict(K=[1, 2], F=F, g=g, A=base.matrix(np.ones((1, 2))), b=base.matrix(np.ones(2))),
            "'b' must be a dense 'd' matrix of size (1,1)")]
    for kw, msg in bad:
        with pytest.raises(TypeError) as e:
            solvers.gp(**kw)
        assert str(e.value) == msg


def test_forms_not_carried_raise_with_their_names():
    c = base.matrix(np.ones(2))
    F = lambda x=None, z=None: (0, base.matrix(np.zeros(2)))
    G, h = base.matrix(np.eye(2)), base.matrix(np.ones(2))
    op = lambda x, y, trans="N", alpha=1.0, beta=0.0: None
    cases = [(dict(dims={"l": 0, "q": [2], "s": []}), "'q' or 's' cones"), (dict(dims={"l": 0, "q": [], "s": [1]}), "'q' or 's' cones"),
             (dict(kktsolver="ldl"), "kktsolver"), (dict(kktsolver=lambda x, z, W: None), "kktsolver"),
             (dict(G=op), "operator-form"), (dict(A=op), "operator-form"), (dict(xnewcopy=base.matrix), "vector hooks"),
             (dict(ydot=lambda a, b: 0.0), "vector hooks")]
    for kw, word in cases:
        args = dict(G=G, h=h)
        args.update(kw)
        for call in (lambda: solvers.cpl(c, F, **args), lambda: solvers.cp(F, **args)):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert word in str(e.value)
    # operator-form Df and H: a callback that returns functions (met at the first evaluation, before a device is asked for)
    Dfop = lambda u, v, alpha=1.0, beta=0.0, trans="N": None
    Fdf = lambda x=None, z=None: (1, base.matrix(np.zeros(2))) if x is None else (np.zeros(1), Dfop, np.zeros((2, 2)))
    Fh = lambda x=None, z=None: (1, base.matrix(np.zeros(2))) if x is None else (np.zeros(1), np.zeros((1, 2)), Dfop)
    for Fop, word in ((Fdf, "second"), (Fh, "third")):
        with pytest.raises(NotImplementedError) as e:
            solvers.cpl(c, Fop, G, h)
        assert "operator-form" in str(e.value) and word in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        solvers.gp([1], base.matrix(np.ones((1, 2))), base.matrix(np.zeros(1)), kktsolver="chol")
    assert "kktsolver" in str(e.value)


@pytest.mark.parametrize("name", G23_CASES)
def test_gp_plan_patterns_equal_a_numpy_restatement(name):
    """Df: row i holds the columns met by block i; H: the lower pattern of F' blockdiag(11') F."""
    K, n, Fp, Fi, Fx = g23_ccs(name)
    ev = cvx.GPEval(K, n, Fp, Fi, Fx, G23[name + "__g"])
    assert_plan_patterns(ev, K, n, Fp, Fi)


def test_gp_plan_argument_checks():
    L = _lib.lib()
    h = ctypes.c_void_p()
    K = np.array([2, 1], dtype=np.int64)
    Fp, Fi = np.array([0, 2, 3], dtype=np.int64), np.array([0, 0, 2], dtype=np.int64)        # (0, 0) stored twice
    assert L.kvx_gp_plan(2, _lib.pi(K), 2, _lib.pi(Fp), _lib.pi(Fi), ctypes.byref(h)) == _lib.KVX_EINVAL
    assert b"twice" in L.kvx_last_error()
    Fi = np.array([0, 3, 2], dtype=np.int64)                                                 # row 3 of 3
    assert L.kvx_gp_plan(2, _lib.pi(K), 2, _lib.pi(Fp), _lib.pi(Fi), ctypes.byref(h)) == _lib.KVX_EINVAL
    K0 = np.array([2, 0], dtype=np.int64)
    assert L.kvx_gp_plan(2, _lib.pi(K0), 2, _lib.pi(Fp), _lib.pi(Fi), ctypes.byref(h)) == _lib.KVX_EINVAL
    assert L.kvx_gp_plan(0, _lib.pi(K), 2, _lib.pi(Fp), _lib.pi(Fi), ctypes.byref(h)) == _lib.KVX_EINVAL
    Fi = np.array([1, 0, 2], dtype=np.int64)                                                 # rows unsorted inside a column: accepted
    assert L.kvx_gp_plan(2, _lib.pi(K), 2, _lib.pi(Fp), _lib.pi(Fi), ctypes.byref(h)) == _lib.KVX_OK
    assert L.kvx_gp_pattern(None, None, None, None, None, None, None) == _lib.KVX_EINVAL
    assert L.kvx_gp_eval_dev(None, None, None, None, None, None, None, None) == _lib.KVX_EINVAL
    L.kvx_gp_free(h)
    L.kvx_gp_free(None)


def test_gp_evaluation_fails_loudly_without_gpu():
    """kvx_gp_eval_dev has no host arithmetic behind it: without a HIP device it answers KVX_EDEVICE and the drivers raise."""
    if _lib.lib().kvx_device_count() > 0:
        pytest.skip("GPU present")
    L = _lib.lib()
    K, n, Fp, Fi, Fx = g23_ccs("k312")
    ev = cvx.GPEval(K, n, Fp, Fi, Fx, G23["k312__g"])
    buf = np.zeros(64)
    ptr = buf.ctypes.data
    assert L.kvx_gp_eval_dev(ev._h, ptr, ptr, ptr, None, ptr, ptr, None) == _lib.KVX_EDEVICE
    assert b"no CPU fallback" in L.kvx_last_error()
    with pytest.raises(RuntimeError):
        solvers.gp([int(k) for k in K], base.matrix(G23["k312__F"]), base.matrix(G23["k312__g"]), options={"show_progress": False})
    F = lambda x=None, z=None: (0, base.matrix(np.zeros(2))) if x is None else (0.0, np.zeros((1, 2)), np.zeros((2, 2)))
    with pytest.raises(RuntimeError):
        solvers.cp(F, options={"show_progress": False})


def test_goldens_come_from_the_reference():
    assert "reference" in str(G23["via"])
    assert set(G23_CASES) >= {"k1", "k111", "k312", "k63_64_65_1", "k300_2", "spread700", "sparse", "k5_40_1_n20"}
    assert [int(k) for k in G23["k63_64_65_1__K"]] == [63, 64, 65, 1] and [int(k) for k in G23["k300_2__K"]] == [300, 2]
    y = G23["spread700__F"] @ G23["spread700__x"] + G23["spread700__g"]
    assert y.max() > 700 and y.min() < -700
    S = G23["sparse__F"]
    assert bool(G23["sparse__sparse"]) and not S[:, 2].any() and np.flatnonzero(S[3:5].any(axis=0)).tolist() == [0]
    for name in G23_CASES:
        assert G23[name + "__f"].shape == G23[name + "__K"].shape
        assert G23[name + "__Df"].shape == (G23[name + "__K"].size, G23[name + "__F"].shape[1])
    meta = json.load(open(os.path.join(_GOLD, "g24_cvx_programs.json")))
    Z = np.load(os.path.join(_GOLD, "g24_cvx_programs.npz"))
    assert "reference" in meta["via"]
    assert set(meta["cases"]) == {"gp_doc", "cp_acent", "cp_robls", "cpl_floorplan", "gp_random", "gp_doc_maxiters", "gp_edges"}
    assert meta["cases"]["gp_doc_maxiters"]["status"] == "unknown"
    assert all(m["status"] == "optimal" for k, m in meta["cases"].items() if k != "gp_doc_maxiters")
    for name in meta["cases"]:
        assert Z[name + "__sol_x"].size > 0
    assert meta["cases"]["gp_edges"]["K"] == [257, 17, 16] and Z["gp_edges__F"].shape == (290, 17)
    assert np.array_equal(Z["gp_edges__g"][257:], np.concatenate([np.full(k, -1.0 - np.log(k)) for k in (17, 16)]))
