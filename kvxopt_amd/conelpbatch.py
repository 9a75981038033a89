"""Many small dense cone programs over all three kinds of cone in one launch, with infeasibility certificates:

    conelp_batch(c, G, h, dims, A=None, b=None, options=None) -> dict          also kvxopt_amd.solvers.conelp_batch

solves  minimize c_b'x  s.t.  G_b x + s = h_b, A_b x = b_b, s in K  for b = 0..B-1 with
K = R^ml_+ x Q^{q_0} x ... x Q^{q_nq-1} x S^{m_0}_+ x ... x S^{m_ns-1}_+ given by dims = {'l': ml, 'q': [q_0, ...], 's': [m_0, ...]},
the same for every member, rows stacked as in conelp: the 'l' rows first, then the 'q' cones, then every 's' block as its
m_k x m_k matrix in column-major order.  Only the lower triangle of an 's' block is read, in G's columns and in h, as the reference
does.  It is the algorithm of solvers.conelp (the self-dual embedding, coneprog.py:662-1436, with the Nesterov-Todd scaling of the
'q' and 's' blocks, misc.py:290-419, 467-634, and the Newton systems of misc.kkt_chol2 on W^-T G), one workgroup per member from its
starting point to its status or its certificate (csrc/conelp_batch.hip, kvx_conelp_batch_solve).  It completes the family
lp_batch / qp_batch / socp_batch / sdp_batch with the members that have more than one kind of cone: robust MPC with norm bounds and
an LMI terminal set, grasp checks with friction cones and a stiffness LMI, relaxations of branch-and-bound nodes with bounds, norm
cuts and a moment block.

conelp_batch always runs its own kernel, whichever kinds are present.  lp_batch, socp_batch and sdp_batch are the faster entries for
their cones (DESIGN 17 has the cost of generality), and a member's bytes are those of the kernel that solves it: the specialised
entries and this one agree to rounding, not to the bit.

  c        n x B, member b in column b; defines n and B
  h, b     N x B and p x B with N = ml + sum(q_k) + sum(m_k^2), or one column shared by all members
  G, A     each one matrix shared by all members (base.matrix, base.spmatrix or a 2-D array; sparse input is made dense on the
           host) or a float64 array (B, rows, n) with member b in [b]
  dims     checked as conelp checks it (_ipm.check_dims)
  limits   1 <= n <= 64, 1 <= N <= 384, ml >= 0, 0 <= nq <= 128, every q_k >= 1, 0 <= ns <= 32, 1 <= m_k <= 16, 0 <= p <= n, and
           conelp's rank condition on the packed dimension, p + ml + sum(q_k) + sum(m_k (m_k + 1) / 2) >= n (coneprog.py:512, 572):
           a ValueError outside them -- solvers.conelp is the path for larger problems, and solvers.socp_batch for a batch
           without 's' blocks whose N is above 384.  There is no fallback loop.
  options  maxiters, abstol, reltol, feastol as solvers.conelp checks them; refinement must be 0, which is the default here
           when the key is absent, whereas solvers.conelp defaults to 1; show_progress is accepted and nothing is printed.
           The module-level solvers.options is not read.  No primalstart / dualstart, no kktsolver, no solver=.

Member b's result is what _ipm.conelp_start plus _ipm.conelp_loop give on that member alone with refinement 0, the dense kkt_chol2
solve and mu = (|lmbda|^2 + lmbda_g^2) / (1 + Nd) with Nd = ml + sum(q_k) + sum(m_k), the length of lmbda (coneprog.py:1248).
Every kind of row is treated as its own batch solver treats it: see kvxopt_amd.lpbatch for the 'l' rows and the loop,
kvxopt_amd.socpbatch for the 'q' rows and kvxopt_amd.sdpbatch for the 's' rows.  max_step, the two pushes and the slacks are taken
over the whole cone; S = Gs'Gs [+ A'A] is one Gram matrix over the scaled rows of all three kinds; kkt_chol2's F['singular'] branch
is carried per member as in lp_batch.  Fixed summation order, no atomics; a member's bytes do not depend on B, on its place or on
the other members.

The result has the keys, NaN conventions and `exit` codes 0-5 of lp_batch; 's' and 'z' are N x B with every 's' block a full
symmetric matrix, as cone.conelp returns them; 'primal slack' and 'dual slack' are the reference's -max_step over the whole cone."""
from . import _batch
from ._batch import LP_STATS as _STATS
from ._batch import MAX_CONE_ROWS as MAX_ROWS
from ._batch import MAX_M, MAX_N, MAX_NQ, MAX_NS, STATUS

_limit = _batch.limiter("conelp_batch", "conelp")


def _prepare(c, G, h, dims, A, b, options):
    """Every argument check, on the host; returns what kvx_conelp_batch_solve takes."""
    opt, dims = _batch.options("conelp_batch", "conelp", options, dims, "'l', 'q' and 's'", qp=False)
    ml, q, s = int(dims["l"]), [int(k) for k in dims["q"]], [int(k) for k in dims["s"]]
    c, n, B = _batch.members(c, "c")
    _limit("n", n, 1, MAX_N)
    _limit("nq", len(q), 0, MAX_NQ)
    _limit("ns", len(s), 0, MAX_NS)
    for m in s:
        _limit("m_k", m, 1, MAX_M)
    N = ml + sum(q) + sum(m * m for m in s)
    if s:
        _limit("N", N, 1, MAX_ROWS)
    else:
        _limit("N", N, 1, MAX_ROWS, "solvers.socp_batch solves batches without 's' blocks up to N = 512, solvers.conelp one problem "
                                    "of any size")
    Gv, sG, rows = _batch.matrix(G, "G", n, B, defines="c")
    if rows != N:
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (N, n))
    hv, sh = _batch.shared_or_batch(h, "h", N, B, "'h' must be a 'd' matrix of size (%d,1)" % N)
    p, eqA, eqb = _batch.equalities(A, b, n, B, "c", _limit)
    packed = ml + sum(q) + sum(m * (m + 1) // 2 for m in s)
    if p + packed < n:
        raise ValueError("conelp_batch: p + ml + sum(q_k) + sum(m_k (m_k + 1) / 2) = %d is outside its limit, at least n = %d "
                         "(conelp's Rank([G; A]) < n); solvers.conelp raises the same for one problem" % (p + packed, n))
    return opt, (B, n, ml, q, s, N, p), (_batch.flat(c, B), (Gv, sG), (hv, sh), eqA, eqb)


def conelp_batch(c, G, h, dims, A=None, b=None, options=None):
    opt, (B, n, ml, q, s, N, p), data = _prepare(c, G, h, dims, A, b, options)
    return _batch.solve("kvx_conelp_batch_solve", [B, n, ml] + _batch.orders(q) + _batch.orders(s) + [p], data, opt, B, n, p, N, _STATS, STATUS)
