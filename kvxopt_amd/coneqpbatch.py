"""Many small dense cone QPs over all three kinds of cone in one launch:

    coneqp_batch(P, q, G, h, dims, A=None, b=None, options=None) -> dict          also kvxopt_amd.solvers.coneqp_batch

solves  minimize (1/2) x'P_b x + q_b'x  s.t.  G_b x + s = h_b, A_b x = b_b, s in K  for b = 0..B-1 with
K = R^ml_+ x Q^{q_0} x ... x Q^{q_nq-1} x S^{m_0}_+ x ... x S^{m_ns-1}_+ given by dims = {'l': ml, 'q': [q_0, ...], 's': [m_0, ...]},
the same for every member, rows stacked as conelp_batch stacks them: the 'l' rows first, then the 'q' cones, then every 's' block as
its m_k x m_k matrix in column-major order.  Only the lower triangle of an 's' block is read, in G's columns and in h, and only the
lower triangle of P.  It is the algorithm of solvers.coneqp (coneprog.py:2044-2547: no embedding, one KKT solve per direction, the
Mehrotra correction; the Nesterov-Todd scaling of the 'q' and 's' blocks, misc.py:290-419, 467-634; the Newton systems of
misc.kkt_chol with H = P), one workgroup per member from its starting point to its status (csrc/coneqp_batch.hip,
kvx_coneqp_batch_solve).  It is qp_batch with cones: an MPC step with a tracking cost, norm bounds and an LMI terminal set, grasp
and contact QPs with friction cones, portfolio sweeps with a risk cone, projection layers onto cone-representable sets.

coneqp_batch always runs its own kernel, whichever kinds are present: qp_batch is the faster entry for the orthant alone, and the two
agree to rounding, not to the bit.

  q        n x B, member b in column b; defines n and B
  h, b     N x B and p x B with N = ml + sum(q_k) + sum(m_k^2), or one column shared by all members
  P, G, A  each one matrix shared by all members (base.matrix, base.spmatrix or a 2-D array; sparse input is made dense on the
           host) or a float64 array (B, rows, n) with member b in [b]; only the lower triangle of P is read
  dims     checked as coneqp checks it (_ipm.check_dims)
  limits   those of conelp_batch: 1 <= n <= 64, 1 <= N <= 384, ml >= 0, 0 <= nq <= 128, every q_k >= 1, 0 <= ns <= 32,
           1 <= m_k <= 16, 0 <= p <= n: a ValueError outside them -- solvers.coneqp is the path for larger problems.  There is no
           rank condition on the packed dimension: P may supply the rank, and a member without it ends with exit 3.  There is no
           fallback loop.
  options  maxiters, abstol, reltol, feastol, use_correction as solvers.coneqp checks them; refinement must be 0, which is the
           default here when the key is absent, whereas solvers.coneqp defaults to 1 with 'q' or 's' cones; show_progress is
           accepted and nothing is printed.  The module-level solvers.options is not read.  No initvals, no kktsolver.

Member b's result is what _ipm.coneqp_start plus _ipm.coneqp_loop give on that member alone with refinement 0, the dense kkt_chol
system S = P + Gs'Gs with Gs = W^-T G, K = X'X, and mu = gap / (ml + nq + sum(m_k)).  As in qp_batch and cone.coneqp there is no A'A
repair.  Every kind of row is treated as conelp_batch treats it (kvxopt_amd.lpbatch, socpbatch, sdpbatch); max_step, the two pushes
and the slacks are taken over the whole cone.  Fixed summation order, no atomics; a member's bytes do not depend on B, on its place
or on the other members.

The result has the keys, NaN conventions and `exit` codes of qp_batch: 0 optimal, 1 maxiters reached, 2 singular KKT matrix after the
first iteration, 3 the factorisation with W = I or the first one failed (solvers.coneqp raises ValueError("Rank(A) < p or
Rank([P; A; G]) < n")): that member has zeros in x, y, s, z, 0 iterations and nan statistics, and does not disturb the others.  's'
and 'z' are N x B with every 's' block a full symmetric matrix, as cone.coneqp returns them; 'primal slack' and 'dual slack' are the
reference's -max_step over the whole cone."""
from . import _batch
from ._batch import EXIT_OPTIMAL, MAX_M, MAX_N, MAX_NQ, MAX_NS  # noqa: F401
from ._batch import MAX_CONE_ROWS as MAX_ROWS
from ._batch import QP_STATS as _STATS

_limit = _batch.limiter("coneqp_batch", "coneqp")


def _prepare(P, q, G, h, dims, A, b, options):
    """Every argument check, on the host; returns what kvx_coneqp_batch_solve takes."""
    opt, dims = _batch.options("coneqp_batch", "coneqp", options, dims, "'l', 'q' and 's'", qp=True)
    ml, qd, sd = int(dims["l"]), [int(k) for k in dims["q"]], [int(k) for k in dims["s"]]
    q, n, B = _batch.members(q, "q")
    _limit("n", n, 1, MAX_N)
    _limit("nq", len(qd), 0, MAX_NQ)
    _limit("ns", len(sd), 0, MAX_NS)
    for m in sd:
        _limit("m_k", m, 1, MAX_M)
    N = ml + sum(qd) + sum(m * m for m in sd)
    _limit("N", N, 1, MAX_ROWS)
    Pv, sP, _ = _batch.matrix(P, "P", n, B, rows=n)
    Gv, sG, rows = _batch.matrix(G, "G", n, B)
    if rows != N:
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (N, n))
    hv, sh = _batch.shared_or_batch(h, "h", N, B, "'h' must be a 'd' matrix of size (%d,1)" % N)
    p, eqA, eqb = _batch.equalities(A, b, n, B, "q", _limit)
    return opt, (B, n, ml, qd, sd, N, p), ((Pv, sP), _batch.flat(q, B), (Gv, sG), (hv, sh), eqA, eqb)


def coneqp_batch(P, q, G, h, dims, A=None, b=None, options=None):
    opt, (B, n, ml, qd, sd, N, p), data = _prepare(P, q, G, h, dims, A, b, options)
    return _batch.solve("kvx_coneqp_batch_solve", [B, n, ml] + _batch.orders(qd) + _batch.orders(sd) + [p], data, opt, B, n, p, N, _STATS, _batch.QP_STATUS,
                        correction=True)
