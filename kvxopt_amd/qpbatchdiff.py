"""Derivatives of a solved batch of small dense quadratic programs:

    qp_batch_vjp(P, q, G, h, A=None, b=None, *, sol, gx, wrt=("P", "q", "G", "h", "A", "b"), options=None) -> dict
    qp_batch_jvp(P, q, G, h, A=None, b=None, *, sol, dP=None, dq=None, dG=None, dh=None, dA=None, db=None, options=None) -> dict

also kvxopt_amd.solvers.qp_batch_vjp / qp_batch_jvp.  `sol` is what qp_batch returned for the same problem arguments.  At the
returned x, y, s, z of member b the differentiated KKT conditions are a linear system with the matrix

    K = [ P  A'  G' ;  A  0  0 ;  G  0  -diag(s / z) ],

the Newton matrix qp_batch factors at every iteration, so a derivative costs one assembly, one Cholesky factorisation and a few
substitutions per member, about one interior-point iteration (csrc/qp_batch_diff.hip: one workgroup per member, one launch;
kvx_qp_batch_vjp / kvx_qp_batch_jvp).  The mathematics is that of Amos & Kolter, "OptNet" (2017), section 3.

  reverse  given gx = dl/dx (n x B), K [ux; uy; uz] = [-gx; 0; 0]; then dl/dq = ux, dl/dh = -uz, dl/db = -uy,
           dl/dP = (ux x' + x ux') / 2 (the full symmetric matrix: the gradient with respect to a symmetric P),
           dl/dG = uz x' + z ux', dl/dA = uy x' + y ux'.
           The result has 'ux' (n x B), 'uy' (p x B), 'uz' (ml x B), 'exit' (B) and for each name in `wrt` the gradient in the
           shape the argument was given: a (B, rows, n) matrix argument gets a (B, rows, n) gradient, columns get columns; a
           matrix all members share, or a shared column h or b, gets the SUM over the members as one item (a 2-D array; a
           vector where the column was given as a vector).  The gradient of q is n x B.  Matrix gradients not named in `wrt`
           are not formed on the device.  With p = 0 the gradients of A and b are None.
  forward  given perturbations dP (symmetric, its lower triangle read, as P is), dq, dG, dh, dA, db -- each None (zero), one
           item shared by all members, or per member, in the shapes qp_batch accepts for P .. b --
           K [dx; dy; dz] = [-(dP x + dq + dG'z + dA'y); db - dA x; dh - dG x] and ds = -(s / z) dz.
           The result has 'x', 'y', 'z', 's' (the directional derivatives, shaped as in `sol`) and 'exit'.
  exit     0 done; 1 skipped because the member's sol['exit'] is not 0; 2 a pivot failed or some s_k, z_k is not positive and
           finite.  A member with 1 or 2 has zeros in every output and adds nothing to a shared sum; the others are undisturbed.
  options  only 'refinement': 0 to 3 steps of iterative refinement, default 1.

Two numerical facts.  Rounding: every entry of s / z is far from 1, tiny on active rows and huge on inactive ones, and the
reduced Cholesky solve alone is off by 1e-9 to 1e-4 relative, the more the tighter the solution; a refinement step forms the
residual of the full 3 x 3 system in float64 and solves again with the same factors, which brings 1e-15 to 1e-7; so the default
is 1, and 2 is the choice for solutions at tolerances near 1e-10.  Truncation: the derivative is that of the solution handed in,
a point of the central path, not of the exact QP.  At the default abstol / reltol / feastol of qp_batch members with a weakly
active row (s_k and z_k both moderate) differ from the derivative of the exact QP by up to 6e-2, single members by 5e-1; at 1e-10
they agree with central differences.  For derivatives solve with tolerances near 1e-8 to 1e-9; float64 members can then end
with exit 2 at the limit of their precision, and are skipped here.

The limits and the texts of the argument checks are those of qp_batch.  Every check runs before a device is asked for; there is
no CPU fallback.  Not carried: several cotangents per call, derivatives of lp_batch / gp_batch (coneqp_batch: coneqpbatchdiff), gradients with
respect to y and z, the derivative fused into the forward launch, a torch.autograd.Function."""
import numpy as np

from . import _lib, qpbatch

EXIT_DONE, EXIT_SKIPPED, EXIT_FAILED = range(3)
MAX_REFINEMENT = 3
WRT = ("P", "q", "G", "h", "A", "b")


def _refinement(who, options):
    o = dict(options or {})
    ref = o.pop("refinement", 1)
    if o:
        raise ValueError("%s: options accepts only 'refinement', not %s" % (who, ", ".join(repr(k) for k in sorted(o, key=str))))
    if isinstance(ref, bool) or not isinstance(ref, (int, np.integer)) or ref < 0:
        raise ValueError("options['refinement'] must be a nonnegative integer")
    if ref > MAX_REFINEMENT:
        raise ValueError("%s: options['refinement'] = %d is outside its limit 0 <= refinement <= %d" % (who, ref, MAX_REFINEMENT))
    return int(ref)


def _problem(who, P, q, G, h, A, b):
    """qp_batch's own checks of the problem arguments, under the entry's name."""
    try:
        _, dims, data = qpbatch._prepare(P, q, G, h, A, b, None)
    except ValueError as e:
        raise ValueError(str(e).replace("qp_batch:", who + ":", 1)) from None
    return dims, data


def _solution(sol, B, n, ml, p):
    """x, y, s, z and exit of `sol` as contiguous arrays, one member after the other."""
    if not isinstance(sol, dict) or any(k not in sol for k in ("x", "y", "s", "z", "exit")):
        raise TypeError("'sol' must be the dictionary qp_batch returned, with 'x', 'y', 's', 'z' and 'exit'")
    out = []
    for k, rows in (("x", n), ("y", p), ("s", ml), ("z", ml)):
        v = np.asarray(sol[k], dtype=np.float64)
        if v.shape != (rows, B):
            raise TypeError("sol['%s'] must be a 'd' matrix of size (%d, %d)" % (k, rows, B))
        out.append(np.ascontiguousarray(v.T).reshape(-1))
    code = np.asarray(sol["exit"])
    if code.shape != (B,) or code.dtype.kind not in "iu":
        raise TypeError("sol['exit'] must be an integer array of length %d" % B)
    return out, np.ascontiguousarray(code, dtype=np.int64)


def _common(dims, data, vecs, code, ref):
    """The leading arguments of all four C entries: sizes, P, G, A with strides, the solution, the refinement."""
    (Pv, sP), _, (Gv, sG), _, (Av, sA), _ = data
    x, y, s, z = vecs
    p = dims[3]
    return list(dims) + [_lib.pd(Pv), sP, _lib.pd(Gv), sG, _lib.pd(Av) if p else None, sA,
                         _lib.pd(x), _lib.pd(y) if p else None, _lib.pd(s), _lib.pd(z), _lib.pi(code), ref]


def _from_members(v, shared, rows, n, B):
    """A matrix gradient as the C entry wrote it -- column-major, one member after the other -- in the argument's shape."""
    return np.ascontiguousarray(v.reshape(n, rows).T) if shared else np.ascontiguousarray(v.reshape(B, n, rows).transpose(0, 2, 1))


def _column_gradient(g, given, shared, done):
    """The gradient of h or b: per member, or the sum over the done members in the shape the shared column was given."""
    if not shared:
        return g
    t = g[:, done].sum(axis=1)
    return t.reshape(-1, 1) if isinstance(given, np.ndarray) and given.ndim == 2 else t


def qp_batch_vjp(P, q, G, h, A=None, b=None, *, sol, gx, wrt=WRT, options=None):
    who = "qp_batch_vjp"
    ref = _refinement(who, options)
    dims, data = _problem(who, P, q, G, h, A, b)
    B, n, ml, p = dims
    vecs, code = _solution(sol, B, n, ml, p)
    g = qpbatch._columns(gx, "gx", "one column per member")
    if g.shape != (n, B):
        raise TypeError("'gx' must be a 'd' matrix of size (%d, %d)" % (n, B))
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    if any(k not in WRT for k in wrt):
        raise ValueError("%s: wrt names %s; it takes 'P', 'q', 'G', 'h', 'A', 'b'" % (who, ", ".join(repr(k) for k in wrt if k not in WRT)))
    gv = np.ascontiguousarray(g.T).reshape(-1)
    sP, sG, sA = data[0][1], data[2][1], data[4][1]
    L = _lib.lib()
    ux, uy, uz = (np.zeros((rows, B), order="F") for rows in (n, p, ml))
    gexit = np.zeros(B, dtype=np.int64)
    mats = {}
    for k, rows, stride in (("P", n, sP), ("G", ml, sG), ("A", p, sA)):
        mats[k] = np.zeros((B if stride else 1) * rows * n) if k in wrt and rows else None
    args = _common(dims, data, vecs, code, ref)
    args += [_lib.pd(gv), _lib.pd(ux), _lib.pd(uy) if p else None, _lib.pd(uz)]
    args += [None if mats[k] is None else _lib.pd(mats[k]) for k in ("P", "G", "A")] + [_lib.pi(gexit)]
    _lib.raise_for(L.kvx_qp_batch_vjp(*args), "kvx_qp_batch_vjp")
    out = {"ux": ux, "uy": uy, "uz": uz, "exit": gexit}
    done = gexit == EXIT_DONE
    for k in wrt:
        if k == "q":
            out[k] = ux.copy()
        elif k == "h":
            out[k] = _column_gradient(0.0 - uz, h, data[3][1] == 0, done)            # 0 - u: no negative zeros
        elif k == "b":
            out[k] = _column_gradient(0.0 - uy, b, data[5][1] == 0, done) if p else None
        else:
            rows, stride = {"P": (n, sP), "G": (ml, sG), "A": (p, sA)}[k]
            out[k] = None if mats[k] is None else _from_members(mats[k], stride == 0, rows, n, B)
    return out


def _perturbation(name, v, like, n, B, rows):
    """(values or None, member stride) of one perturbation, checked as qp_batch checks the datum it perturbs."""
    if v is None:
        return None, 0
    if like in ("P", "G", "A"):
        vals, stride, _ = qpbatch._matrix(v, name, n, B, rows=rows)
        return vals, stride
    return qpbatch._shared_or_batch(v, name, rows, B, "'%s' must be a 'd' matrix of size (%d,1)" % (name, rows))


def qp_batch_jvp(P, q, G, h, A=None, b=None, *, sol, dP=None, dq=None, dG=None, dh=None, dA=None, db=None, options=None):
    who = "qp_batch_jvp"
    ref = _refinement(who, options)
    dims, data = _problem(who, P, q, G, h, A, b)
    B, n, ml, p = dims
    vecs, code = _solution(sol, B, n, ml, p)
    pert = [_perturbation("d" + k, v, k, n, B, rows)
            for k, v, rows in (("P", dP, n), ("q", dq, n), ("G", dG, ml), ("h", dh, ml), ("A", dA, p), ("b", db, p))]
    L = _lib.lib()
    dx, dy, dz, ds = (np.zeros((rows, B), order="F") for rows in (n, p, ml, ml))
    gexit = np.zeros(B, dtype=np.int64)
    args = _common(dims, data, vecs, code, ref)
    for k, (vals, stride) in zip(WRT, pert):
        args += [None if vals is None or (k in "Ab" and not p) else _lib.pd(vals), stride]
    args += [_lib.pd(dx), _lib.pd(dy) if p else None, _lib.pd(dz), _lib.pd(ds), _lib.pi(gexit)]
    _lib.raise_for(L.kvx_qp_batch_jvp(*args), "kvx_qp_batch_jvp")
    return {"x": dx, "y": dy, "z": dz, "s": ds, "exit": gexit}
