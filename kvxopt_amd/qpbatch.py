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
import numpy as np

from . import _ipm, _lib, base

MAX_N, MAX_ML = 64, 512
EXIT_OPTIMAL, EXIT_MAXITERS, EXIT_SINGULAR, EXIT_RANK = range(4)
_STATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility",
          "primal slack", "dual slack")


def _columns(v, name, what):
    """A vector argument as a 2-D float64 array, one member per column."""
    a = v.a if isinstance(v, base.matrix) else v
    if not isinstance(a, np.ndarray):
        a = base.flat(a)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2:
        raise TypeError("'%s' must be a 'd' matrix with %s" % (name, what))
    return a


def _matrix(M, name, n, B, rows=None):
    """(values, member stride, rows) of a matrix argument: one member column-major after the other; stride 0 for a shared matrix."""
    if isinstance(M, np.ndarray) and M.ndim != 2:
        if M.ndim != 3 or M.dtype != np.float64:
            raise TypeError("'%s' must be one matrix or a float64 array of shape (B, rows, %d)" % (name, n))
        if M.shape[0] != B:
            raise TypeError("'%s' has %d members, 'q' has %d columns" % (name, M.shape[0], B))
        m = M.shape[1]
        if M.shape[2] != n or (rows is not None and m != rows):
            raise TypeError(_size_text(name, rows, n))
        return np.ascontiguousarray(M.transpose(0, 2, 1)).reshape(-1), m * n, m
    if isinstance(M, np.ndarray):
        (m, nc), D = M.shape, np.ascontiguousarray(np.asarray(M, dtype=np.float64).T)
    else:
        m, nc, cp, ri, v = base.ccs(M)
        D = np.zeros((nc, m))
        D[np.repeat(np.arange(nc, dtype=np.int64), np.diff(cp)), ri] = v
    if nc != n or (rows is not None and m != rows):
        raise TypeError(_size_text(name, rows, n))
    return D.reshape(-1), 0, m


def _size_text(name, rows, n):
    if name == "A":
        return "'A' must be a 'd' matrix with %d columns" % n                      # _ipm.problem's texts
    return "'%s' must be a 'd' matrix of size (%s, %d)" % (name, "%d" % rows if rows is not None else "ml", n)


def _limit(name, value, lo, hi):
    if not lo <= value <= hi:
        raise ValueError("qp_batch: %s = %d is outside its limit %d <= %s <= %s; solvers.qp solves one problem of any size"
                         % (name, value, lo, name, "n" if name == "p" else "%d" % hi))


def _shared_or_batch(v, name, rows, B, text):
    a = _columns(v, name, "%d rows" % rows)
    if a.shape[0] != rows:
        raise TypeError(text)
    if a.shape[1] not in (1, B):
        raise TypeError("'%s' must have one column or B = %d columns" % (name, B))
    return np.ascontiguousarray(a.T).reshape(-1), (rows if a.shape[1] == B and B > 1 else 0)


def _prepare(P, q, G, h, A, b, options):
    """Every argument check, on the host; returns what kvx_qp_batch_solve takes."""
    opt = _ipm.options(options, {}, qp=True)
    if opt.refinement != 0:
        raise NotImplementedError("qp_batch: options['refinement'] = %d is not carried, only 0 (the orthant's default); "
                                  "solvers.qp refines" % opt.refinement)
    q = _columns(q, "q", "one column per member")
    n, B = q.shape
    if B < 1:
        raise TypeError("'q' must have at least one column")
    _limit("n", n, 1, MAX_N)
    Pv, sP, _ = _matrix(P, "P", n, B, rows=n)
    Gv, sG, ml = _matrix(G, "G", n, B)
    _limit("ml", ml, 1, MAX_ML)
    hv, sh = _shared_or_batch(h, "h", ml, B, "'h' must be a 'd' matrix of size (%d,1)" % ml)
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
    return opt, (B, n, ml, p), ((Pv, sP), (qv, n if B > 1 else 0), (Gv, sG), (hv, sh), (Av, sA), (bv, sb))


def qp_batch(P, q, G, h, A=None, b=None, options=None):
    opt, (B, n, ml, p), data = _prepare(P, q, G, h, A, b, options)
    L = _lib.lib()
    x, y, s, z = (np.zeros((rows, B), order="F") for rows in (n, p, ml, ml))
    stats = np.zeros((len(_STATS), B), order="F")
    iters, code = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    args = [B, n, ml, p]
    for v, stride in data:
        args += [None if v is None else _lib.pd(v), stride]
    args += [int(opt.maxiters), float(opt.abstol), float(opt.reltol), float(opt.feastol), int(opt.correction)]
    args += [_lib.pd(x), _lib.pd(y) if p else None, _lib.pd(s), _lib.pd(z), _lib.pd(stats), _lib.pi(iters), _lib.pi(code)]
    _lib.raise_for(L.kvx_qp_batch_solve(*args), "kvx_qp_batch_solve")
    sol = {"status": ["optimal" if c == EXIT_OPTIMAL else "unknown" for c in code], "x": x, "y": y, "s": s, "z": z}
    sol.update((k, stats[i].copy()) for i, k in enumerate(_STATS))
    sol.update({"iterations": iters, "exit": code})
    return sol
