"""The Python front of the batch entries (qp_batch, lp_batch, socp_batch, sdp_batch, conelp_batch, coneqp_batch, gp_batch and, through
_batchdiff, their derivatives), written once: the argument helpers with their texts, the limit refusal, the refinement preamble, the
equality block, the flattened linear term, and the call into the C entry with the result dictionary.  An entry's module keeps its
docstring, its own limits and texts, its `dims`, its rank condition and the head of its C argument list.  This module imports none
of them."""
import numpy as np

from . import _ipm, _lib, base

MAX_N, MAX_ML = 64, 512                                    # the orthant entries; 512 is also socp_batch's N
MAX_CONE_ROWS, MAX_NQ, MAX_NS, MAX_M = 384, 128, 32, 16    # the entries with 's' blocks; 128 is also socp_batch's nq
EXIT_OPTIMAL, EXIT_MAXITERS, EXIT_SINGULAR, EXIT_RANK, EXIT_PRIMAL_INFEASIBLE, EXIT_DUAL_INFEASIBLE = range(6)
QP_STATUS = {EXIT_OPTIMAL: "optimal"}                      # coneqp's loop: everything else is "unknown"
STATUS = {EXIT_OPTIMAL: "optimal", EXIT_PRIMAL_INFEASIBLE: "primal infeasible", EXIT_DUAL_INFEASIBLE: "dual infeasible"}
QP_STATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility",
            "primal slack", "dual slack")
LP_STATS = QP_STATS + ("residual as primal infeasibility certificate", "residual as dual infeasibility certificate")


def columns(v, name, what):
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


def matrix(M, name, n, B, rows=None, defines="q"):
    """(values, member stride, rows) of a matrix argument: one member column-major after the other; stride 0 for a shared matrix.
    defines: the name of the argument whose columns are the members."""
    if isinstance(M, np.ndarray) and M.ndim != 2:
        if M.ndim != 3 or M.dtype != np.float64:
            raise TypeError("'%s' must be one matrix or a float64 array of shape (B, rows, %d)" % (name, n))
        if M.shape[0] != B:
            raise TypeError("'%s' has %d members, '%s' has %d columns" % (name, M.shape[0], defines, B))
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


def shared_or_batch(v, name, rows, B, text):
    a = columns(v, name, "%d rows" % rows)
    if a.shape[0] != rows:
        raise TypeError(text)
    if a.shape[1] not in (1, B):
        raise TypeError("'%s' must have one column or B = %d columns" % (name, B))
    return np.ascontiguousarray(a.T).reshape(-1), (rows if a.shape[1] == B and B > 1 else 0)


def limiter(entry, reference):
    """limit(name, value, lo, hi[, other]) of one entry: a ValueError outside lo <= value <= hi that names the entry and, unless
    `other` says otherwise, the solver for one problem of any size."""
    def limit(name, value, lo, hi, other="solvers.%s solves one problem of any size" % reference):
        if not lo <= value <= hi:
            raise ValueError("%s: %s = %d is outside its limit %d <= %s <= %s; %s"
                             % (entry, name, value, lo, name, "n" if name == "p" else "%d" % hi, other))
    return limit


_ORTHANT = object()


def options(entry, reference, user, dims=_ORTHANT, keys=None, **qp):
    """The checked options of an entry, whose 'refinement' must be 0.  Without dims: an orthant entry, where 0 is the reference's
    default too.  Otherwise 0 is the default here when the key is absent; with `keys` (the text that names them) `dims` is the
    caller's and is checked first.  Returns the options, and the checked dims where there are any."""
    if dims is _ORTHANT:
        opt, where, refines = _ipm.options(user, {}, **qp), "the orthant's default", "refines"
    else:
        user = dict(user or {})
        if user.get("refinement") is None:
            user["refinement"] = 0
        if keys is not None:
            if not isinstance(dims, dict):
                raise TypeError("'dims' must be a dictionary with the keys %s" % keys)
            dims = _ipm.check_dims(dims)
        opt, where, refines = _ipm.options(user, dims, **qp), "the default here", "refines, once by default"
    if opt.refinement != 0:
        raise NotImplementedError("%s: options['refinement'] = %d is not carried, only 0 (%s); solvers.%s %s"
                                  % (entry, opt.refinement, where, reference, refines))
    return opt if dims is _ORTHANT else (opt, dims)


def members(v, name):
    """The argument whose columns are the members, and its shape."""
    v = columns(v, name, "one column per member")
    if v.shape[1] < 1:
        raise TypeError("'%s' must have at least one column" % name)
    return (v,) + v.shape


def flat(v, B):
    """(values, member stride) of the argument whose columns are the members."""
    return np.ascontiguousarray(v.T).reshape(-1), v.shape[0] if B > 1 else 0


def equalities(A, b, n, B, defines, limit, absent="'b' must have length 0", length="'b' must have length %d"):
    """p, (A's values, stride), (b's values, stride) of the equality constraints; both None where p = 0."""
    if A is None:
        p, Av, sA = 0, None, 0
        if b is not None and columns(b, "b", "0 rows").shape[0] != 0:
            raise TypeError(absent)
        bv, sb = None, 0
    else:
        Av, sA, p = matrix(A, "A", n, B, defines=defines)
        limit("p", p, 0, n)
        if p == 0:
            Av, bv, sA, sb = None, None, 0, 0
        else:
            if b is None:
                raise TypeError(length % p)
            bv, sb = shared_or_batch(b, "b", p, B, length % p)
    return p, (Av, sA), (bv, sb)


def orders(v):
    """[count, pointer or NULL] of a list of cone or block orders for a C entry; the pointer keeps its array alive."""
    return [len(v), _lib.pi(np.asarray(v, dtype=np.int64)) if v else None]


def pointers(data):
    """[pointer or NULL, member stride, ...] of (values, stride) pairs."""
    args = []
    for v, stride in data:
        args += [None if v is None else _lib.pd(v), stride]
    return args


def solve(symbol, head, data, opt, B, n, p, rows, stats, status, correction=False):
    """The C entry `symbol` on head + data + options + results; the `sol` dictionary of the entry with 's' and 'z' of `rows` rows."""
    L = _lib.lib()
    x, y, s, z = (np.zeros((r, B), order="F") for r in (n, p, rows, rows))
    st = np.zeros((len(stats), B), order="F")
    iters, code = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    args = list(head) + pointers(data)
    args += [int(opt.maxiters), float(opt.abstol), float(opt.reltol), float(opt.feastol)] + ([int(opt.correction)] if correction else [])
    args += [_lib.pd(x), _lib.pd(y) if p else None, _lib.pd(s), _lib.pd(z), _lib.pd(st), _lib.pi(iters), _lib.pi(code)]
    _lib.raise_for(getattr(L, symbol)(*args), symbol)
    sol = {"status": [status.get(int(k), "unknown") for k in code], "x": x, "y": y, "s": s, "z": z}
    sol.update((k, st[i].copy()) for i, k in enumerate(stats))
    sol.update({"iterations": iters, "exit": code})
    return sol
