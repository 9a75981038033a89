"""Many small dense geometric programs in one launch:

    gp_batch(K, F, g, G=None, h=None, A=None, b=None, options=None) -> dict          also kvxopt_amd.solvers.gp_batch

solves  minimize log sum exp(F0_b x + g0_b)  s.t.  log sum exp(Fi_b x + gi_b) <= 0 (i = 1..mnl),  G_b x <= h_b,  A_b x = b_b  for
b = 0..B-1 by the algorithm of solvers.gp (cvxprog.gp -> cp -> cpl, cvxprog.py:1967-2155, 1359-1964, 35-1356; the Newton systems of
misc.kkt_chol2), one workgroup per member from x = 0 to its status (csrc/gp_batch.hip, kvx_gp_batch_solve).  solvers.gp solves
one sparse program per call and pays its host control flow, several host reads per line-search trial and about 150 launches per
iteration whatever the size; this entry is for the other kind of user: gate and wire sizing swept over corners, power control
per channel realisation, floor-planning and design-space sweeps, GP layers inside a learning loop.

  K        one list of positive ints for all members: block i has K[i] terms, block 0 is the objective; l = sum(K), mnl = len(K) - 1
  g        l x B, member b in column b; defines B
  F, G, A  each one matrix shared by all members (base.matrix, base.spmatrix or a 2-D array; sparse input is made dense on the
           host) or a float64 array (B, rows, n) with member b in [b]; F has l rows and defines n; G and A may be None
  h, b     ml x B and p x B, or one column shared by all members
  limits   1 <= n <= 63, N = mnl + 1 + ml <= 192, l <= 768, 0 <= p <= n, and 160 KiB of LDS (every shape inside the other limits
           fits): a ValueError outside them -- solvers.gp is the path for larger problems
  options  maxiters, abstol, reltol, feastol as solvers.gp checks them; refinement must be 0, which is the default here
           (solvers.gp defaults to 1); show_progress is accepted and nothing is printed.  The module-level solvers.options is not
           read.  No kktsolver.

Member b's result is what cvx._cpl gives on that member alone at refinement 0: cp's epigraph form (t is column n of the member's
system) from x = 0, t = 0, s = z = 1, with a dense Cholesky KKT and no A'A repair.

The result has 'status' (B strings, "optimal" or "unknown"), 'x' (n x B), 'y' (p x B), 'znl', 'snl' (mnl x B, the objective row
dropped), 'zl', 'sl' (ml x B), float arrays of length B 'gap', 'relative gap' (nan where the reference returns None), 'primal
objective', 'dual objective', 'primal infeasibility', 'dual infeasibility', 'primal slack', 'dual slack', and int arrays
'iterations' and 'exit': 0 optimal, 1 maxiters reached, 2 singular KKT matrix after the first iteration, 3 the first factorisation
failed (solvers.gp raises ValueError("Rank(A) < p or Rank([H(x); A; Df(x); G]) < n")): that member has zeros in its vectors, 0
iterations and nan statistics, 4 a line search did not end within 64 halvings of its step (the reference has no bound): the last
accepted iterate is returned.  A member does not disturb the others: its bytes do not depend on B, on its place or on the other
members."""
import numpy as np

from . import _batch, base
from ._batch import EXIT_OPTIMAL  # noqa: F401
from ._batch import QP_STATS as _STATS

MAX_N, MAX_ROWS, MAX_L = 63, 192, 768
EXIT_MAXITERS, EXIT_SINGULAR, EXIT_RANK, EXIT_LINESEARCH = 1, 2, 3, 4

_limit = _batch.limiter("gp_batch", "gp")
_columns, _matrix, _shared_or_batch = _batch.columns, _batch.matrix, _batch.shared_or_batch


def _shape(M):
    return tuple(M.shape[-2:]) if isinstance(M, np.ndarray) else tuple(M.size)


def _is_mat(M):
    return isinstance(M, (base.matrix, base.spmatrix)) or (isinstance(M, np.ndarray) and M.ndim in (2, 3))


def _is_d(M):
    return getattr(M, "typecode", "d") == "d" and (not isinstance(M, np.ndarray) or M.dtype == np.float64)


def _prepare(K, F, g, G, h, A, b, options):
    """Every argument check, on the host; returns what kvx_gp_batch_solve takes."""
    opt, _ = _batch.options("gp_batch", "gp", options, {"l": 0, "q": [], "s": []})
    if type(K) is not list or not K or [k for k in K if type(k) is not int or k <= 0]:       # cvx.gp_problem's texts
        raise TypeError("'K' must be a list of positive integers")
    l, mnl = sum(K), len(K) - 1
    if not _is_mat(F) or not _is_d(F) or _shape(F)[0] != l:
        raise TypeError("'F' must be a dense or sparse 'd' matrix with %d rows" % l)
    n = _shape(F)[1]
    g = _columns(g, "g", "%d rows, one column per member" % l)
    if g.shape[0] != l:
        raise TypeError("'g' must be a 'd' matrix with %d rows, one column per member" % l)
    B = g.shape[1]
    if B < 1:
        raise TypeError("'g' must have at least one column")
    for M, name in ((F, "F"), (G, "G"), (A, "A")):
        if M is not None and (not _is_mat(M) or not _is_d(M) or _shape(M)[1] != n):
            raise TypeError("'%s' must be a dense or sparse 'd' matrix with %d columns" % (name, n))
        if isinstance(M, np.ndarray) and M.ndim == 3 and M.shape[0] != B:
            raise TypeError("'%s' has %d members, 'g' has %d columns" % (name, M.shape[0], B))
    _limit("n", n, 1, MAX_N)
    _limit("l", l, 1, MAX_L)
    ml = 0 if G is None else _shape(G)[0]
    _limit("N", mnl + 1 + ml, 1, MAX_ROWS)
    Fv, sF, _ = _matrix(F, "F", n, B, rows=l)
    if ml == 0:
        Gv, sG, hv, sh = None, 0, None, 0
        if h is not None and _columns(h, "h", "0 rows").shape[0] != 0:
            raise TypeError("'h' must be a dense 'd' matrix of size (0,1)")
    else:
        Gv, sG, _ = _matrix(G, "G", n, B)
        if h is None:
            raise TypeError("'h' must be a dense 'd' matrix of size (%d,1)" % ml)
        hv, sh = _shared_or_batch(h, "h", ml, B, "'h' must be a dense 'd' matrix of size (%d,1)" % ml)
    # an A without rows is an absent one, so b is looked at; every text of A's own has been raised above
    p, eqA, eqb = _batch.equalities(A if A is not None and _shape(A)[0] else None, b, n, B, "g", _limit,
                                    "'b' must be a dense 'd' matrix of size (0,1)", "'b' must be a dense 'd' matrix of size (%d,1)")
    return opt, (B, n, list(K), ml, p), ((Fv, sF), _batch.flat(g, B), (Gv, sG), (hv, sh), eqA, eqb)


def gp_batch(K, F, g, G=None, h=None, A=None, b=None, options=None):
    opt, (B, n, K, ml, p), data = _prepare(K, F, g, G, h, A, b, options)
    m = len(K)
    sol = _batch.solve("kvx_gp_batch_solve", [B, n, m - 1, _batch.orders(K)[1], ml, p], data, opt, B, n, p, m + ml, _STATS, _batch.QP_STATUS)
    s, z = sol.pop("s"), sol.pop("z")
    out = {k: sol.pop(k) for k in ("status", "x", "y")}
    out.update({"znl": np.asfortranarray(z[1:m]), "snl": np.asfortranarray(s[1:m]), "zl": np.asfortranarray(z[m:]),
                "sl": np.asfortranarray(s[m:])})
    out.update(sol)
    return out
