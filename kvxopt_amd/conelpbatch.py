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
import numpy as np

from . import _ipm, _lib
from .lpbatch import _STATS, _lp_matrix, STATUS
from .qpbatch import MAX_N, _columns, _shared_or_batch

MAX_ROWS = 384
MAX_NQ = 128
MAX_NS = 32
MAX_M = 16


def _limit(name, value, lo, hi, other="solvers.conelp solves one problem of any size"):
    if not lo <= value <= hi:
        raise ValueError("conelp_batch: %s = %d is outside its limit %d <= %s <= %s; %s"
                         % (name, value, lo, name, "n" if name == "p" else "%d" % hi, other))


def _prepare(c, G, h, dims, A, b, options):
    """Every argument check, on the host; returns what kvx_conelp_batch_solve takes."""
    user = dict(options or {})
    if user.get("refinement") is None:
        user["refinement"] = 0
    if not isinstance(dims, dict):
        raise TypeError("'dims' must be a dictionary with the keys 'l', 'q' and 's'")
    dims = _ipm.check_dims(dims)
    opt = _ipm.options(user, dims, qp=False)
    if opt.refinement != 0:
        raise NotImplementedError("conelp_batch: options['refinement'] = %d is not carried, only 0 (the default here); "
                                  "solvers.conelp refines, once by default" % opt.refinement)
    ml, q, s = int(dims["l"]), [int(k) for k in dims["q"]], [int(k) for k in dims["s"]]
    c = _columns(c, "c", "one column per member")
    n, B = c.shape
    if B < 1:
        raise TypeError("'c' must have at least one column")
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
    Gv, sG, rows = _lp_matrix(G, "G", n, B)
    if rows != N:
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (N, n))
    hv, sh = _shared_or_batch(h, "h", N, B, "'h' must be a 'd' matrix of size (%d,1)" % N)
    if A is None:
        p, Av, sA = 0, None, 0
        if b is not None and _columns(b, "b", "0 rows").shape[0] != 0:
            raise TypeError("'b' must have length 0")
        bv, sb = None, 0
    else:
        Av, sA, p = _lp_matrix(A, "A", n, B)
        _limit("p", p, 0, n)
        if p == 0:
            Av, bv, sA, sb = None, None, 0, 0
        else:
            if b is None:
                raise TypeError("'b' must have length %d" % p)
            bv, sb = _shared_or_batch(b, "b", p, B, "'b' must have length %d" % p)
    packed = ml + sum(q) + sum(m * (m + 1) // 2 for m in s)
    if p + packed < n:
        raise ValueError("conelp_batch: p + ml + sum(q_k) + sum(m_k (m_k + 1) / 2) = %d is outside its limit, at least n = %d "
                         "(conelp's Rank([G; A]) < n); solvers.conelp raises the same for one problem" % (p + packed, n))
    cv = np.ascontiguousarray(c.T).reshape(-1)
    return opt, (B, n, ml, q, s, N, p), ((cv, n if B > 1 else 0), (Gv, sG), (hv, sh), (Av, sA), (bv, sb))


def conelp_batch(c, G, h, dims, A=None, b=None, options=None):
    opt, (B, n, ml, q, s, N, p), data = _prepare(c, G, h, dims, A, b, options)
    L = _lib.lib()
    x, y, sv, z = (np.zeros((rows, B), order="F") for rows in (n, p, N, N))
    stats = np.zeros((len(_STATS), B), order="F")
    iters, code = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    qv, mv = np.asarray(q, dtype=np.int64), np.asarray(s, dtype=np.int64)
    args = [B, n, ml, len(q), _lib.pi(qv) if q else None, len(s), _lib.pi(mv) if s else None, p]
    for v, stride in data:
        args += [None if v is None else _lib.pd(v), stride]
    args += [int(opt.maxiters), float(opt.abstol), float(opt.reltol), float(opt.feastol)]
    args += [_lib.pd(x), _lib.pd(y) if p else None, _lib.pd(sv), _lib.pd(z), _lib.pd(stats), _lib.pi(iters), _lib.pi(code)]
    _lib.raise_for(L.kvx_conelp_batch_solve(*args), "kvx_conelp_batch_solve")
    sol = {"status": [STATUS.get(int(k), "unknown") for k in code], "x": x, "y": y, "s": sv, "z": z}
    sol.update((k, stats[i].copy()) for i, k in enumerate(_STATS))
    sol.update({"iterations": iters, "exit": code})
    return sol
