"""Many small dense semidefinite programs in one launch, with infeasibility certificates:

    sdp_batch(c, G, h, dims, A=None, b=None, options=None) -> dict          also kvxopt_amd.solvers.sdp_batch

solves  minimize c_b'x  s.t.  G_b x + s = h_b, A_b x = b_b, s in K  for b = 0..B-1 with K = R^ml_+ x S^{m_0}_+ x ... x S^{m_ns-1}_+
given by dims = {'l': ml, 's': [m_0, ...]}, the same for every member, rows stacked as in conelp: the 'l' rows first, then every
block as its m_k x m_k matrix in column-major order.  Only the lower triangle of a block is read, in G's columns and in h, as the
reference does.  It is the algorithm of solvers.sdp (conelp's self-dual embedding, coneprog.py:662-1436, with the Nesterov-Todd
scaling of the 's' blocks, misc.py:354-419, 582-634, misc_solvers.c:188-240, 343-397, 700-770, 845-882, 1029-1046, 1086-1160, and
the Newton systems of misc.kkt_chol2 on W^-T G), one workgroup per member from its starting point to its status or its certificate
(csrc/sdp_batch.hip, kvx_sdp_batch_solve).  It adds the semidefinite cone to the family lp_batch / qp_batch / socp_batch: LMI and
Lyapunov checks over a grid of operating points, low-degree moment and sum-of-squares relaxations per sample, max-cut and
Lovasz-theta relaxations of the small subgraphs of a branch-and-bound tree, minimum-volume ellipsoids per window.

  c        n x B, member b in column b; defines n and B
  h, b     N x B and p x B with N = ml + sum(m_k^2), or one column shared by all members
  G, A     each one matrix shared by all members (base.matrix, base.spmatrix or a 2-D array; sparse input is made dense on the
           host) or a float64 array (B, rows, n) with member b in [b]
  dims     checked as conelp checks it (_ipm.check_dims); dims['q'] must be absent or empty
  limits   1 <= n <= 64, 1 <= N <= 384, ml >= 0, 0 <= ns <= 32, 1 <= m_k <= 16, 0 <= p <= n, and conelp's rank condition on the
           packed dimension, p + ml + sum(m_k (m_k + 1) / 2) >= n (coneprog.py:512, 572): a ValueError outside them -- solvers.sdp
           is the path for larger problems.  There is no fallback loop.
  options  maxiters, abstol, reltol, feastol as solvers.sdp checks them; refinement must be 0, which is the default here
           when the key is absent, whereas solvers.sdp defaults to 1; show_progress is accepted and nothing is printed.
           The module-level solvers.options is not read.  No primalstart / dualstart, no kktsolver, no solver=.

Member b's result is what _ipm.conelp_start plus _ipm.conelp_loop give on that member alone with refinement 0, the dense kkt_chol2
solve and mu = (|lmbda|^2 + lmbda_g^2) / (1 + Nd) with Nd = ml + sum(m_k), the length of lmbda (coneprog.py:1248): see
kvxopt_amd.lpbatch for the 'l' rows and the loop; on the 's' rows max_step is minus the smallest eigenvalue, the pushes add to the
diagonals, W_k x = r_k' x r_k with r_k, rti_k and lmbda_k from the Cholesky factors of s_k, z_k and the singular values of Lz'Ls,
ds = lmbda o lmbda with the corrector's -sigma mu e on the diagonals, sinv with the diagonal lmbda, W'ds in the right-hand side,
ws3 = (ds dz + dz ds) / 2, scale2 before the step bound, whose eigen-decompositions of ds and dz the update of r_k, rti_k and
lmbda_k consumes, then s = W'lmbda, z = W^-1 lmbda and gap = (|lmbda| / tau)^2.  kkt_chol2's F['singular'] branch is carried as in
lp_batch.  A block of s or z that is not positive definite when the first scaling is computed ends its member with exit 3.
Fixed summation order, no atomics; a member's bytes do not depend on B, on its place or on the other members.

The result has the keys, NaN conventions and `exit` codes 0-5 of lp_batch; 's' and 'z' are N x B with every 's' block a full
symmetric matrix, as cone.conelp returns them; 'primal slack' and 'dual slack' are the reference's -max_step over the whole cone."""
from . import _batch
from ._batch import LP_STATS as _STATS
from ._batch import MAX_CONE_ROWS as MAX_ROWS
from ._batch import MAX_M, MAX_N, MAX_NS, STATUS

_limit = _batch.limiter("sdp_batch", "sdp")


def _prepare(c, G, h, dims, A, b, options):
    """Every argument check, on the host; returns what kvx_sdp_batch_solve takes."""
    opt, dims = _batch.options("sdp_batch", "sdp", options, dims, "'l' and 's'", qp=False)
    if dims["q"]:
        raise ValueError("sdp_batch: dims['q'] = %r is outside its limit, absent or empty; solvers.socp_batch solves batches with "
                         "second-order cones and solvers.conelp problems with both kinds" % (dims["q"],))
    ml, s = int(dims["l"]), [int(k) for k in dims["s"]]
    c, n, B = _batch.members(c, "c")
    _limit("n", n, 1, MAX_N)
    _limit("ns", len(s), 0, MAX_NS)
    for m in s:
        _limit("m_k", m, 1, MAX_M)
    N = ml + sum(m * m for m in s)
    _limit("N", N, 1, MAX_ROWS)
    Gv, sG, rows = _batch.matrix(G, "G", n, B, defines="c")
    if rows != N:
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (N, n))
    hv, sh = _batch.shared_or_batch(h, "h", N, B, "'h' must be a 'd' matrix of size (%d,1)" % N)
    p, eqA, eqb = _batch.equalities(A, b, n, B, "c", _limit)
    packed = ml + sum(m * (m + 1) // 2 for m in s)
    if p + packed < n:
        raise ValueError("sdp_batch: p + ml + sum(m_k (m_k + 1) / 2) = %d is outside its limit, at least n = %d (conelp's "
                         "Rank([G; A]) < n); solvers.sdp raises the same for one problem" % (p + packed, n))
    return opt, (B, n, ml, s, N, p), (_batch.flat(c, B), (Gv, sG), (hv, sh), eqA, eqb)


def sdp_batch(c, G, h, dims, A=None, b=None, options=None):
    opt, (B, n, ml, s, N, p), data = _prepare(c, G, h, dims, A, b, options)
    return _batch.solve("kvx_sdp_batch_solve", [B, n, ml] + _batch.orders(s) + [p], data, opt, B, n, p, N, _STATS, STATUS)
