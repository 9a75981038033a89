"""Many small dense second-order-cone programs in one launch, with infeasibility certificates:

    socp_batch(c, G, h, dims, A=None, b=None, options=None) -> dict          also kvxopt_amd.solvers.socp_batch

solves  minimize c_b'x  s.t.  G_b x + s = h_b, A_b x = b_b, s in K  for b = 0..B-1 with K = R^ml_+ x Q^{m_0} x ... x Q^{m_nq-1}
given by dims = {'l': ml, 'q': [m_0, ...]}, the same for every member, rows stacked as in conelp: the 'l' rows first, then the
cones in order.  It is the algorithm of solvers.socp (conelp's self-dual embedding, coneprog.py:662-1436, with the Nesterov-Todd
scaling of the 'q' blocks, misc.py:290-352, 467-580, misc_solvers.c:144-186, 301-341, 671-700, 803-835, 1073-1085, and the Newton
systems of misc.kkt_chol2 on W^-T G), one workgroup per member from its starting point to its status or its certificate
(csrc/socp_batch.hip, kvx_socp_batch_solve).  It completes the family lp_batch / qp_batch / socp_batch: robust MPC horizons,
friction-cone and grasp checks, robust least squares over many windows, portfolio members with a risk bound, norm-constrained
relaxations of sibling branch-and-bound nodes.

  c        n x B, member b in column b; defines n and B
  h, b     N x B and p x B with N = ml + sum(m_k), or one column shared by all members
  G, A     each one matrix shared by all members (base.matrix, base.spmatrix or a 2-D array; sparse input is made dense on the
           host) or a float64 array (B, rows, n) with member b in [b]
  dims     checked as conelp checks it (_ipm.check_dims); dims['s'] must be absent or empty
  limits   1 <= n <= 64, 1 <= N <= 512, ml >= 0, 0 <= nq <= 128, every m_k >= 1, 0 <= p <= n, and conelp's p + N >= n: a
           ValueError outside them -- solvers.socp is the path for larger problems.  There is no fallback loop.
  options  maxiters, abstol, reltol, feastol as solvers.socp checks them; refinement must be 0, which is the default here
           when the key is absent, whereas solvers.socp defaults to 1; show_progress is accepted and nothing is printed.
           The module-level solvers.options is not read.  No primalstart / dualstart, no kktsolver, no solver=.

Member b's result is what _ipm.conelp_start plus _ipm.conelp_loop give on that member alone with refinement 0, the dense kkt_chol2
solve and mu = |lmbda|^2 / (1 + N) as coneprog.py:1248 forms it (1 + cdim_diag, the length of lmbda, not 1 + ml + nq): see
kvxopt_amd.lpbatch for the 'l' rows and the loop; on the 'q' rows max_step is |u_1| - u_0, the pushes add to u_0 only,
W_k = beta_k (2 v_k v_k' - J) and lmbda_k are formed as the reference forms them (jnrm2 as sqrt(x_0 - |x_1|) sqrt(x_0 + |x_1|)),
ds = lmbda o lmbda by sprod with the corrector's -sigma mu e on the first entry of each cone, sinv, W'ds in the right-hand side,
ws3 = ds o dz, scale2 before the step bound, update_scaling of v_k, beta_k, lmbda_k, then s = W'lmbda, z = W^-1 lmbda and
gap = (|lmbda| / tau)^2.  kkt_chol2's F['singular'] branch is carried as in lp_batch.  Fixed
summation order, no atomics; a member's bytes do not depend on B, on its place or on the other members.

The result has the keys, NaN conventions and `exit` codes 0-5 of lp_batch; 's' and 'z' are N x B; 'primal slack' and 'dual
slack' are the reference's -max_step over the whole cone."""
from . import _batch
from ._batch import LP_STATS as _STATS
from ._batch import MAX_ML as MAX_ROWS
from ._batch import MAX_N, MAX_NQ, STATUS

_limit = _batch.limiter("socp_batch", "socp")


def _prepare(c, G, h, dims, A, b, options):
    """Every argument check, on the host; returns what kvx_socp_batch_solve takes."""
    opt, dims = _batch.options("socp_batch", "socp", options, dims, "'l' and 'q'", qp=False)
    if dims["s"]:
        raise ValueError("socp_batch: dims['s'] = %r is outside its limit, absent or empty; solvers.sdp and solvers.conelp solve "
                         "problems with semidefinite blocks" % (dims["s"],))
    ml, q = int(dims["l"]), [int(k) for k in dims["q"]]
    c, n, B = _batch.members(c, "c")
    _limit("n", n, 1, MAX_N)
    _limit("nq", len(q), 0, MAX_NQ)
    N = ml + sum(q)
    _limit("N", N, 1, MAX_ROWS)
    Gv, sG, rows = _batch.matrix(G, "G", n, B, defines="c")
    if rows != N:
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (N, n))
    hv, sh = _batch.shared_or_batch(h, "h", N, B, "'h' must be a 'd' matrix of size (%d,1)" % N)
    p, eqA, eqb = _batch.equalities(A, b, n, B, "c", _limit)
    if p + N < n:
        raise ValueError("socp_batch: p + N = %d is outside its limit p + N >= n = %d (conelp's Rank([G; A]) < n); solvers.socp "
                         "raises the same for one problem" % (p + N, n))
    return opt, (B, n, ml, q, N, p), (_batch.flat(c, B), (Gv, sG), (hv, sh), eqA, eqb)


def socp_batch(c, G, h, dims, A=None, b=None, options=None):
    opt, (B, n, ml, q, N, p), data = _prepare(c, G, h, dims, A, b, options)
    return _batch.solve("kvx_socp_batch_solve", [B, n, ml] + _batch.orders(q) + [p], data, opt, B, n, p, N, _STATS, STATUS)
