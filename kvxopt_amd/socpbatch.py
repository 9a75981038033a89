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
import numpy as np

from . import _ipm, _lib
from .lpbatch import _STATS, _lp_matrix, STATUS
from .qpbatch import MAX_ML as MAX_ROWS, MAX_N, _columns, _shared_or_batch

MAX_NQ = 128


def _limit(name, value, lo, hi):
    if not lo <= value <= hi:
        raise ValueError("socp_batch: %s = %d is outside its limit %d <= %s <= %s; solvers.socp solves one problem of any size"
                         % (name, value, lo, name, "n" if name == "p" else "%d" % hi))


def _prepare(c, G, h, dims, A, b, options):
    """Every argument check, on the host; returns what kvx_socp_batch_solve takes."""
    user = dict(options or {})
    if user.get("refinement") is None:
        user["refinement"] = 0
    if not isinstance(dims, dict):
        raise TypeError("'dims' must be a dictionary with the keys 'l' and 'q'")
    dims = _ipm.check_dims(dims)
    opt = _ipm.options(user, dims, qp=False)
    if opt.refinement != 0:
        raise NotImplementedError("socp_batch: options['refinement'] = %d is not carried, only 0 (the default here); "
                                  "solvers.socp refines, once by default" % opt.refinement)
    if dims["s"]:
        raise ValueError("socp_batch: dims['s'] = %r is outside its limit, absent or empty; solvers.sdp and solvers.conelp solve "
                         "problems with semidefinite blocks" % (dims["s"],))
    ml, q = int(dims["l"]), [int(k) for k in dims["q"]]
    c = _columns(c, "c", "one column per member")
    n, B = c.shape
    if B < 1:
        raise TypeError("'c' must have at least one column")
    _limit("n", n, 1, MAX_N)
    _limit("nq", len(q), 0, MAX_NQ)
    N = ml + sum(q)
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
    if p + N < n:
        raise ValueError("socp_batch: p + N = %d is outside its limit p + N >= n = %d (conelp's Rank([G; A]) < n); solvers.socp "
                         "raises the same for one problem" % (p + N, n))
    cv = np.ascontiguousarray(c.T).reshape(-1)
    return opt, (B, n, ml, q, N, p), ((cv, n if B > 1 else 0), (Gv, sG), (hv, sh), (Av, sA), (bv, sb))


def socp_batch(c, G, h, dims, A=None, b=None, options=None):
    opt, (B, n, ml, q, N, p), data = _prepare(c, G, h, dims, A, b, options)
    L = _lib.lib()
    x, y, s, z = (np.zeros((rows, B), order="F") for rows in (n, p, N, N))
    stats = np.zeros((len(_STATS), B), order="F")
    iters, code = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    qv = np.asarray(q, dtype=np.int64)
    args = [B, n, ml, len(q), _lib.pi(qv) if q else None, p]
    for v, stride in data:
        args += [None if v is None else _lib.pd(v), stride]
    args += [int(opt.maxiters), float(opt.abstol), float(opt.reltol), float(opt.feastol)]
    args += [_lib.pd(x), _lib.pd(y) if p else None, _lib.pd(s), _lib.pd(z), _lib.pd(stats), _lib.pi(iters), _lib.pi(code)]
    _lib.raise_for(L.kvx_socp_batch_solve(*args), "kvx_socp_batch_solve")
    sol = {"status": [STATUS.get(int(k), "unknown") for k in code], "x": x, "y": y, "s": s, "z": z}
    sol.update((k, stats[i].copy()) for i, k in enumerate(_STATS))
    sol.update({"iterations": iters, "exit": code})
    return sol
