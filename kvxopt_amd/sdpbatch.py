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
import numpy as np

from . import _ipm, _lib
from .lpbatch import _STATS, _lp_matrix, STATUS
from .qpbatch import MAX_N, _columns, _shared_or_batch

MAX_ROWS = 384
MAX_NS = 32
MAX_M = 16


def _limit(name, value, lo, hi):
    if not lo <= value <= hi:
        raise ValueError("sdp_batch: %s = %d is outside its limit %d <= %s <= %s; solvers.sdp solves one problem of any size"
                         % (name, value, lo, name, "n" if name == "p" else "%d" % hi))


def _prepare(c, G, h, dims, A, b, options):
    """Every argument check, on the host; returns what kvx_sdp_batch_solve takes."""
    user = dict(options or {})
    if user.get("refinement") is None:
        user["refinement"] = 0
    if not isinstance(dims, dict):
        raise TypeError("'dims' must be a dictionary with the keys 'l' and 's'")
    dims = _ipm.check_dims(dims)
    opt = _ipm.options(user, dims, qp=False)
    if opt.refinement != 0:
        raise NotImplementedError("sdp_batch: options['refinement'] = %d is not carried, only 0 (the default here); "
                                  "solvers.sdp refines, once by default" % opt.refinement)
    if dims["q"]:
        raise ValueError("sdp_batch: dims['q'] = %r is outside its limit, absent or empty; solvers.socp_batch solves batches with "
                         "second-order cones and solvers.conelp problems with both kinds" % (dims["q"],))
    ml, s = int(dims["l"]), [int(k) for k in dims["s"]]
    c = _columns(c, "c", "one column per member")
    n, B = c.shape
    if B < 1:
        raise TypeError("'c' must have at least one column")
    _limit("n", n, 1, MAX_N)
    _limit("ns", len(s), 0, MAX_NS)
    for m in s:
        _limit("m_k", m, 1, MAX_M)
    N = ml + sum(m * m for m in s)
    _limit("N", N, 1, MAX_ROWS)
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
    packed = ml + sum(m * (m + 1) // 2 for m in s)
    if p + packed < n:
        raise ValueError("sdp_batch: p + ml + sum(m_k (m_k + 1) / 2) = %d is outside its limit, at least n = %d (conelp's "
                         "Rank([G; A]) < n); solvers.sdp raises the same for one problem" % (p + packed, n))
    cv = np.ascontiguousarray(c.T).reshape(-1)
    return opt, (B, n, ml, s, N, p), ((cv, n if B > 1 else 0), (Gv, sG), (hv, sh), (Av, sA), (bv, sb))


def sdp_batch(c, G, h, dims, A=None, b=None, options=None):
    opt, (B, n, ml, s, N, p), data = _prepare(c, G, h, dims, A, b, options)
    L = _lib.lib()
    x, y, sv, z = (np.zeros((rows, B), order="F") for rows in (n, p, N, N))
    stats = np.zeros((len(_STATS), B), order="F")
    iters, code = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    mv = np.asarray(s, dtype=np.int64)
    args = [B, n, ml, len(s), _lib.pi(mv) if s else None, p]
    for v, stride in data:
        args += [None if v is None else _lib.pd(v), stride]
    args += [int(opt.maxiters), float(opt.abstol), float(opt.reltol), float(opt.feastol)]
    args += [_lib.pd(x), _lib.pd(y) if p else None, _lib.pd(sv), _lib.pd(z), _lib.pd(stats), _lib.pi(iters), _lib.pi(code)]
    _lib.raise_for(L.kvx_sdp_batch_solve(*args), "kvx_sdp_batch_solve")
    sol = {"status": [STATUS.get(int(k), "unknown") for k in code], "x": x, "y": y, "s": sv, "z": z}
    sol.update((k, stats[i].copy()) for i, k in enumerate(_STATS))
    sol.update({"iterations": iters, "exit": code})
    return sol
