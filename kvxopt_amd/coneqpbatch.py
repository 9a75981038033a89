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
import numpy as np

from . import _ipm, _lib
from .conelpbatch import MAX_M, MAX_NQ, MAX_NS, MAX_ROWS
from .qpbatch import _STATS, EXIT_OPTIMAL, MAX_N, _columns, _matrix, _shared_or_batch


def _limit(name, value, lo, hi):
    if not lo <= value <= hi:
        raise ValueError("coneqp_batch: %s = %d is outside its limit %d <= %s <= %s; solvers.coneqp solves one problem of any size"
                         % (name, value, lo, name, "n" if name == "p" else "%d" % hi))


def _prepare(P, q, G, h, dims, A, b, options):
    """Every argument check, on the host; returns what kvx_coneqp_batch_solve takes."""
    user = dict(options or {})
    if user.get("refinement") is None:
        user["refinement"] = 0
    if not isinstance(dims, dict):
        raise TypeError("'dims' must be a dictionary with the keys 'l', 'q' and 's'")
    dims = _ipm.check_dims(dims)
    opt = _ipm.options(user, dims, qp=True)
    if opt.refinement != 0:
        raise NotImplementedError("coneqp_batch: options['refinement'] = %d is not carried, only 0 (the default here); "
                                  "solvers.coneqp refines, once by default" % opt.refinement)
    ml, qd, sd = int(dims["l"]), [int(k) for k in dims["q"]], [int(k) for k in dims["s"]]
    q = _columns(q, "q", "one column per member")
    n, B = q.shape
    if B < 1:
        raise TypeError("'q' must have at least one column")
    _limit("n", n, 1, MAX_N)
    _limit("nq", len(qd), 0, MAX_NQ)
    _limit("ns", len(sd), 0, MAX_NS)
    for m in sd:
        _limit("m_k", m, 1, MAX_M)
    N = ml + sum(qd) + sum(m * m for m in sd)
    _limit("N", N, 1, MAX_ROWS)
    Pv, sP, _ = _matrix(P, "P", n, B, rows=n)
    Gv, sG, rows = _matrix(G, "G", n, B)
    if rows != N:
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (N, n))
    hv, sh = _shared_or_batch(h, "h", N, B, "'h' must be a 'd' matrix of size (%d,1)" % N)
    if A is None:
        p, Av, sA = 0, None, 0
        if b is not None and _columns(b, "b", "0 rows").shape[0] != 0:
            raise TypeError("'b' must have length 0")
        bv, sb = None, 0
    else:
        Av, sA, p = _matrix(A, "A", n, B)
        _limit("p", p, 0, n)
        if p == 0:
            Av, bv, sA, sb = None, None, 0, 0
        else:
            if b is None:
                raise TypeError("'b' must have length %d" % p)
            bv, sb = _shared_or_batch(b, "b", p, B, "'b' must have length %d" % p)
    qv = np.ascontiguousarray(q.T).reshape(-1)
    return opt, (B, n, ml, qd, sd, N, p), ((Pv, sP), (qv, n if B > 1 else 0), (Gv, sG), (hv, sh), (Av, sA), (bv, sb))


def coneqp_batch(P, q, G, h, dims, A=None, b=None, options=None):
    opt, (B, n, ml, qd, sd, N, p), data = _prepare(P, q, G, h, dims, A, b, options)
    L = _lib.lib()
    x, y, sv, z = (np.zeros((rows, B), order="F") for rows in (n, p, N, N))
    stats = np.zeros((len(_STATS), B), order="F")
    iters, code = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    qv, mv = np.asarray(qd, dtype=np.int64), np.asarray(sd, dtype=np.int64)
    args = [B, n, ml, len(qd), _lib.pi(qv) if qd else None, len(sd), _lib.pi(mv) if sd else None, p]
    for v, stride in data:
        args += [None if v is None else _lib.pd(v), stride]
    args += [int(opt.maxiters), float(opt.abstol), float(opt.reltol), float(opt.feastol), int(opt.correction)]
    args += [_lib.pd(x), _lib.pd(y) if p else None, _lib.pd(sv), _lib.pd(z), _lib.pd(stats), _lib.pi(iters), _lib.pi(code)]
    _lib.raise_for(L.kvx_coneqp_batch_solve(*args), "kvx_coneqp_batch_solve")
    sol = {"status": ["optimal" if c == EXIT_OPTIMAL else "unknown" for c in code], "x": x, "y": y, "s": sv, "z": z}
    sol.update((k, stats[i].copy()) for i, k in enumerate(_STATS))
    sol.update({"iterations": iters, "exit": code})
    return sol
