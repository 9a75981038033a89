"""Many small dense quadratic programs in one launch:

    qp_batch(P, q, G, h, A=None, b=None, options=None) -> dict          also kvxopt_amd.solvers.qp_batch

solves  minimize (1/2) x'P_b x + q_b'x  s.t.  G_b x <= h_b,  A_b x = b_b  for b = 0..B-1 by the algorithm of solvers.qp
(coneprog.py:1762-2547 on the orthant, the Newton systems of misc.kkt_chol2), one workgroup per member from its starting point
to its status (csrc/qp_batch.hip, kvx_qp_batch_solve).  The interior-point drivers of this package solve one large sparse
problem per call and pay about 150 launches per iteration whatever its size; this entry is for the other kind of user: model
predictive control steps, SVM duals on small folds, portfolio sweeps, projection layers.

  q        n x B, member b in column b; defines n and B
  h, b     ml x B and p x B, or one column shared by all members
  P, G, A  each one matrix shared by all members (base.matrix, base.spmatrix or a 2-D array; sparse input is made dense on the
           host) or a float64 array (B, rows, n) with member b in [b]; only the lower triangle of P is read
  limits   1 <= n <= 64, 1 <= ml <= 512, 0 <= p <= n: a ValueError outside them -- solvers.qp is the path for larger problems
  options  maxiters, abstol, reltol, feastol, use_correction as solvers.qp checks them; refinement must be 0 (the orthant's
           default); show_progress is accepted and nothing is printed.  The module-level solvers.options is not read.
           No initvals, no kktsolver.

The result has 'status' (B strings, "optimal" or "unknown"), 'x' (n x B), 'y' (p x B), 's', 'z' (ml x B), float arrays of
length B 'gap', 'relative gap' (nan where the reference returns None), 'primal objective', 'dual objective', 'primal
infeasibility', 'dual infeasibility', 'primal slack', 'dual slack', and int arrays 'iterations' and 'exit': 0 optimal, 1 maxiters
reached, 2 singular KKT matrix after the first iteration, 3 the factorisation with W = I or the first one failed (solvers.qp
raises ValueError("Rank(A) < p or Rank([P; A; G]) < n")): that member has zeros in x, y, s, z, 0 iterations and nan statistics,
and does not disturb the others.  A member's bytes do not depend on B, on its place or on the other members."""
from . import _batch
from ._batch import EXIT_MAXITERS, EXIT_OPTIMAL, EXIT_RANK, EXIT_SINGULAR, MAX_ML, MAX_N  # noqa: F401
from ._batch import QP_STATS as _STATS

_limit = _batch.limiter("qp_batch", "qp")


def _prepare(P, q, G, h, A, b, options):
    """Every argument check, on the host; returns what kvx_qp_batch_solve takes."""
    opt = _batch.options("qp_batch", "qp", options, qp=True)
    q, n, B = _batch.members(q, "q")
    _limit("n", n, 1, MAX_N)
    Pv, sP, _ = _batch.matrix(P, "P", n, B, rows=n)
    Gv, sG, ml = _batch.matrix(G, "G", n, B)
    _limit("ml", ml, 1, MAX_ML)
    hv, sh = _batch.shared_or_batch(h, "h", ml, B, "'h' must be a 'd' matrix of size (%d,1)" % ml)
    p, eqA, eqb = _batch.equalities(A, b, n, B, "q", _limit)
    return opt, (B, n, ml, p), ((Pv, sP), _batch.flat(q, B), (Gv, sG), (hv, sh), eqA, eqb)


def qp_batch(P, q, G, h, A=None, b=None, options=None):
    opt, (B, n, ml, p), data = _prepare(P, q, G, h, A, b, options)
    return _batch.solve("kvx_qp_batch_solve", [B, n, ml, p], data, opt, B, n, p, ml, _STATS, _batch.QP_STATUS, correction=True)
