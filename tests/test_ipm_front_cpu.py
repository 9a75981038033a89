"""The front matter shared by the four interior-point drivers (kvxopt_amd._ipm): option checks, size checks of the problem data
and the refinement default.  Pure host code -- no device is needed, through lp.conelp / lp.coneqp either, because the checks
come before a device is asked for."""
import numpy as np
import pytest

from kvxopt_amd import _ipm, lp
from kvxopt_amd.base import matrix, spmatrix

BAD_OPTIONS = [
    ({"maxiters": 0}, r"options\['maxiters'\] must be a positive integer"),
    ({"maxiters": 2.5}, r"options\['maxiters'\] must be a positive integer"),
    ({"abstol": "x"}, r"options\['abstol'\] must be a scalar"),
    ({"reltol": None}, r"options\['reltol'\] must be a scalar"),
    ({"abstol": 0.0, "reltol": -1.0}, r"at least one of options\['reltol'\] and options\['abstol'\] must be positive"),
    ({"feastol": 0.0}, r"options\['feastol'\] must be a positive scalar"),
    ({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer"),
    ({"refinement": 1.5}, r"options\['refinement'\] must be a nonnegative integer"),
]

G = spmatrix([1.0, 1.0, 1.0], [0, 1, 2], [0, 1, 0], (3, 2))
c, h = matrix([1.0, 1.0]), matrix([1.0, 1.0, 1.0])
P = spmatrix([1.0, 1.0], [0, 1], [0, 1], (2, 2))
A, b = spmatrix([1.0, 1.0], [0, 0], [0, 1], (1, 2)), matrix([1.0])


@pytest.mark.parametrize("bad,text", BAD_OPTIONS)
def test_option_checks(bad, text):
    for qp in (False, True):
        with pytest.raises(ValueError, match=text):
            _ipm.options(bad, {"l": 3}, qp=qp)
    with pytest.raises(ValueError, match=text):
        lp.conelp(c, G, h, options=bad)
    with pytest.raises(ValueError, match=text):
        lp.coneqp(P, c, G, h, options=bad)


def test_option_defaults():
    o = _ipm.options(None, {"l": 3})
    assert (o.maxiters, o.abstol, o.reltol, o.feastol, o.show, o.refinement) == (100, 1e-7, 1e-6, 1e-7, False, 0)
    assert _ipm.options({}, {"l": 1, "q": [3], "s": [2]}).refinement == 1
    assert _ipm.options({"refinement": 2}, {"l": 3}).refinement == 2
    assert _ipm.options({"abstol": -1.0}, {"l": 3}).abstol == -1.0          # one non-positive tolerance is allowed
    assert _ipm.options(None, {"l": 3}, qp=True).correction is True


def test_problem_data():
    pb = _ipm.problem(c, G, h, None, A, b)
    assert (pb.n, pb.p, pb.cdim, pb.dims) == (2, 1, 3, {"l": 3, "q": [], "s": []})
    assert pb.c.dtype == np.float64 and pb.c.flags.c_contiguous and np.array_equal(pb.h, np.ones(3))
    assert np.array_equal(pb.G[0], [0, 2, 3]) and np.array_equal(pb.G[1], [0, 2, 1]) and np.array_equal(pb.A[2], [1.0, 1.0])
    dense = _ipm.problem(np.ones(2), np.asfortranarray(np.ones((3, 2))), np.ones(3), {"l": 1, "q": [2], "s": []}, None, None,
                         np.asfortranarray(np.array([[2.0, 9.0], [1.0, 3.0]])), qp=True)
    assert dense.p == 0 and np.array_equal(dense.A[0], [0, 0, 0]) and dense.b.size == 0
    assert np.array_equal(dense.G[0], [0, 3, 6])                               # a dense matrix keeps every entry
    assert np.array_equal(dense.P[0], [0, 2, 3]) and np.array_equal(dense.P[2], [2.0, 1.0, 3.0])   # lower triangle


SIZE_ERRORS = [
    (dict(h=matrix([1.0, 1.0])), r"'h' must be a 'd' matrix of size \(3,1\)"),
    (dict(c=matrix([1.0, 1.0, 1.0])), r"'G' must be a 'd' matrix of size \(3, 3\)"),
    (dict(A=spmatrix([1.0], [0], [0], (1, 3))), r"'A' must be a 'd' matrix with 2 columns"),
    (dict(b=matrix([1.0, 2.0])), r"'b' must have length 1"),
    (dict(A=None), r"'b' must have length 0"),
]


@pytest.mark.parametrize("change,text", SIZE_ERRORS)
def test_size_errors(change, text):
    kw = dict(c=c, G=G, h=h, A=A, b=b)
    kw.update(change)
    with pytest.raises(TypeError, match=text):
        _ipm.problem(kw["c"], kw["G"], kw["h"], None, kw["A"], kw["b"])
    with pytest.raises(TypeError, match=text):
        lp.conelp(kw["c"], kw["G"], kw["h"], A=kw["A"], b=kw["b"])
    if "c" not in change:                                                      # (with another n the size of P is met first)
        with pytest.raises(TypeError, match=text):
            lp.coneqp(P, kw["c"], kw["G"], kw["h"], A=kw["A"], b=kw["b"])


def test_p_size_and_dims_errors():
    with pytest.raises(TypeError, match=r"'P' must be a 'd' matrix of size \(2, 2\)"):
        lp.coneqp(spmatrix([1.0], [0], [0], (3, 3)), c, G, h)
    with pytest.raises(TypeError, match="'dims\\['q'\\]' must be a list of positive integers"):
        _ipm.problem(c, G, h, {"l": 1, "q": [0, 2], "s": []}, None, None)
    with pytest.raises(TypeError, match="'dims\\['l'\\]' must be a nonnegative integer"):
        _ipm.problem(c, G, h, {"l": -1, "q": [], "s": []}, None, None)
    with pytest.raises(TypeError, match="'dims\\['s'\\]' must be a list of nonnegative integers"):
        _ipm.problem(c, G, h, {"l": 3, "q": [], "s": [-1]}, None, None)


def test_rank_prechecks():
    A3 = spmatrix([1.0, 1.0, 1.0], [0, 1, 2], [0, 1, 0], (3, 2))
    for qp in (False, True):                                                   # p > n
        with pytest.raises(ValueError, match=r"Rank\(A\) < p"):
            _ipm.problem(c, G, h, None, A3, matrix([1.0, 1.0, 1.0]), P if qp else None, qp=qp)
    with pytest.raises(ValueError, match=r"Rank\(A\) < p or Rank\(\[G; A\]\) < n"):
        lp.conelp(c, G, h, A=A3, b=matrix([1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match=r"Rank\(A\) < p or Rank\(\[P; G; A\]\) < n"):
        lp.coneqp(P, c, G, h, A=A3, b=matrix([1.0, 1.0, 1.0]))
    # p + cdim_pckd < n: one 's' block of order 2 packs to 3 rows, n = 5, p = 1
    c5, G5 = np.ones(5), spmatrix([1.0], [0], [0], (4, 5))
    with pytest.raises(ValueError, match=r"Rank\(A\) < p or Rank\(\[G; A\]\) < n"):
        _ipm.problem(c5, G5, np.ones(4), {"l": 0, "q": [], "s": [2]}, spmatrix([1.0], [0], [0], (1, 5)), np.ones(1))
    assert _ipm.problem(c5, G5, np.ones(4), {"l": 0, "q": [], "s": [2]}, None, None, spmatrix([], [], [], (5, 5)), qp=True).n == 5
    with pytest.raises(ValueError, match=r"Rank\(A\) < p or Rank\(\[G; A\]\) < n"):
        lp.conelp(np.ones(3), spmatrix([1.0], [0], [0], (1, 3)), np.ones(1))
