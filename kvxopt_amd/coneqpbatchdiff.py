"""Derivatives of a solved batch of small dense cone QPs:

    coneqp_batch_vjp(P, q, G, h, dims, A=None, b=None, *, sol, gx, wrt=("P", "q", "G", "h", "A", "b"), options=None) -> dict
    coneqp_batch_jvp(P, q, G, h, dims, A=None, b=None, *, sol, dP=None, dq=None, dG=None, dh=None, dA=None, db=None, options=None) -> dict

also kvxopt_amd.solvers.coneqp_batch_vjp / coneqp_batch_jvp.  `sol` is what coneqp_batch returned for the same problem arguments; it
is never modified.  P = 0 is allowed, so this is also the derivative of a cone LP.  The differentiated KKT conditions of member b are a
linear system with the matrix

    K = [ P  A'  G' ;  A  0  0 ;  G  0  -W'W ],        W the Nesterov-Todd scaling of (s, z),

the Newton matrix coneqp_batch factors at every iteration.  For the orthant W'W = diag(s / z) linearises s_k z_k = const exactly at
any interior point (qp_batch_vjp differentiates the returned point as it stands); for 'q' and 's' cones it does so only on the
central path, lmbda o lmbda = mu e, and coneqp_batch returns points with |lmbda o lmbda - mu e|_2 / mu between 1 and 12: the system
at the returned point is off by 1 % to 43 % and does not improve with the tolerance.  So per member (csrc/coneqp_batch_diff.hip: one
workgroup per member, one launch; kvx_coneqp_batch_vjp / kvx_coneqp_batch_jvp):

  1  a member whose sol['exit'] is not 0 is skipped (exit 1);
  2  the scaling is computed from s and z (misc.compute_scaling); if it fails or a value is not finite: exit 2;
  3  at most options['centering'] centring steps are taken with mu = s'z / degree fixed: a Newton step of coneqp with sigma = 1 and no
     Mehrotra term, the full residuals on the right-hand side, the step length min(1, 0.99 / t), the scaling updated as the solver
     updates it; they converge quadratically and stop as soon as |lmbda o lmbda - mu e|_2 <= options['centol'] mu.  A failed pivot:
     exit 2; the threshold not met within the cap: exit 3;
  4  K at the centred point (x, y, s, z, W) is factored as the solver factors it and solved with options['refinement'] steps of
     iterative refinement on the full system in float64.

  reverse  given gx = dl/dx (n x B), K [ux; uy; uz] = [-gx; 0; 0]; then dl/dq = ux, dl/dh = -uz, dl/db = -uy,
           dl/dP = (ux x' + x ux') / 2, dl/dG = uz x' + z ux', dl/dA = uy x' + y ux' with x, y, z of the centred point.
           In the 's' rows z and uz are full symmetric blocks, so rows (i, j) and (j, i) of dl/dG and dl/dh evaluate one expression:
           the gradient with respect to a symmetric argument, the convention dl/dP has.  A user whose free parameters are the lower
           triangle adds the two.
           The result has 'ux' (n x B), 'uy' (p x B), 'uz' (N x B), 'exit', 'centrality', 'centering steps' (B each) and for each name
           in `wrt` the gradient in the shape the argument was given, exactly as qp_batch_vjp returns them: per member where the
           argument was per member, the SUM over the done members for a matrix or column all members share; the gradient of q is
           n x B; matrix gradients not named in `wrt` are not formed on the device; with p = 0 the gradients of A and b are None.
  forward  given perturbations dP, dq, dG, dh, dA, db -- each None (zero), one item shared by all members, or per member, in the
           shapes coneqp_batch accepts for P .. b; of dP and of every 's' block of dG and dh the lower triangle is read and mirrored,
           as in P, G, h -- K [dx; dy; dz] = [-(dP x + dq + dG'z + dA'y); db - dA x; dh - dG x] and ds = -W'W dz.
           The result has 'x', 'y', 'z', 's' (the directional derivatives, shaped as in `sol`), 'exit', 'centrality', 'centering steps'.
  exit     0 done; 1 skipped; 2 the scaling or a pivot failed, or a value is not finite; 3 not centred within the cap.  A member with
           exit != 0 has zeros in every derivative and adds nothing to a sum; the others are undisturbed.
  'centrality'  the final |lmbda o lmbda - mu e|_2 / mu (NaN with exit 1 or 2);  'centering steps'  the steps taken.
  options  only 'refinement' (0 to 3, default 1), 'centering' (0 to 16, default 8) and 'centol' (positive, default 1e-6).
           centering = 0 takes the returned point as it is: the uncentred system.

The tolerance of the solve matters more than for the orthant: solve with abstol = reltol = feastol of 1e-7 to 1e-8.  There float64 and
longdouble restatements of the whole procedure agree to about 1e-6 relative; at 1e-9 single members lose that, and at 1e-10 the float64
Cholesky factor of the scaling fails on several members.  A cone LP (P = 0) solved that tightly sits at a vertex where the reduced
matrix is nearly singular, and a quarter of such members end with exit 2.

The limits and the texts of the argument checks are those of coneqp_batch.  Every check runs before a device is asked for; there is no
CPU fallback.  Not carried: derivatives of conelp_batch (its certificates), gp_batch, socp_batch / sdp_batch as entries of their own,
the centred point as a result, several cotangents per call, a torch binding."""
import numpy as np

from . import _lib, coneqpbatch, qpbatch
from .qpbatchdiff import MAX_REFINEMENT, WRT, _column_gradient, _from_members

EXIT_DONE, EXIT_SKIPPED, EXIT_FAILED, EXIT_NOT_CENTRED = range(4)
MAX_CENTERING = 16
DEFAULT_CENTERING, DEFAULT_CENTOL = 8, 1e-6               # DESIGN 21 has the table they are chosen from


def _options(who, options):
    o = dict(options or {})
    ref, cen, tol = o.pop("refinement", 1), o.pop("centering", DEFAULT_CENTERING), o.pop("centol", DEFAULT_CENTOL)
    if o:
        raise ValueError("%s: options accepts only 'refinement', 'centering' and 'centol', not %s"
                         % (who, ", ".join(repr(k) for k in sorted(o, key=str))))
    for name, v, hi in (("refinement", ref, MAX_REFINEMENT), ("centering", cen, MAX_CENTERING)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("options['%s'] must be a nonnegative integer" % name)
        if v > hi:
            raise ValueError("%s: options['%s'] = %d is outside its limit 0 <= %s <= %d" % (who, name, v, name, hi))
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol > 0:
        raise ValueError("options['centol'] must be a positive scalar")
    return int(ref), int(cen), float(tol)


def _problem(who, P, q, G, h, dims, A, b):
    """coneqp_batch's own checks of the problem arguments, under the entry's name."""
    try:
        _, sizes, data = coneqpbatch._prepare(P, q, G, h, dims, A, b, None)
    except ValueError as e:
        raise ValueError(str(e).replace("coneqp_batch:", who + ":", 1)) from None
    return sizes, data


def _solution(sol, B, n, N, p):
    """x, y, s, z and exit of `sol` as contiguous arrays of their own, one member after the other."""
    if not isinstance(sol, dict) or any(k not in sol for k in ("x", "y", "s", "z", "exit")):
        raise TypeError("'sol' must be the dictionary coneqp_batch returned, with 'x', 'y', 's', 'z' and 'exit'")
    out = []
    for k, rows in (("x", n), ("y", p), ("s", N), ("z", N)):
        v = np.asarray(sol[k], dtype=np.float64)
        if v.shape != (rows, B):
            raise TypeError("sol['%s'] must be a 'd' matrix of size (%d, %d)" % (k, rows, B))
        out.append(np.array(v.T, order="C").reshape(-1))
    code = np.asarray(sol["exit"])
    if code.shape != (B,) or code.dtype.kind not in "iu":
        raise TypeError("sol['exit'] must be an integer array of length %d" % B)
    return out, np.array(code, dtype=np.int64)


def _common(sizes, data, vecs, code, opts):
    """The leading arguments of all four C entries: sizes, the cone, the data with strides, the solution, the options."""
    B, n, ml, qd, sd, N, p = sizes
    qv, mv = np.asarray(qd, dtype=np.int64), np.asarray(sd, dtype=np.int64)
    args = [B, n, ml, len(qd), _lib.pi(qv) if qd else None, len(sd), _lib.pi(mv) if sd else None, p]
    for v, stride in data:
        args += [None if v is None else _lib.pd(v), stride]
    x, y, s, z = vecs
    return args + [_lib.pd(x), _lib.pd(y) if p else None, _lib.pd(s), _lib.pd(z), _lib.pi(code)] + list(opts), (qv, mv)


def coneqp_batch_vjp(P, q, G, h, dims, A=None, b=None, *, sol, gx, wrt=WRT, options=None):
    who = "coneqp_batch_vjp"
    opts = _options(who, options)
    sizes, data = _problem(who, P, q, G, h, dims, A, b)
    B, n, ml, qd, sd, N, p = sizes
    vecs, code = _solution(sol, B, n, N, p)
    g = qpbatch._columns(gx, "gx", "one column per member")
    if g.shape != (n, B):
        raise TypeError("'gx' must be a 'd' matrix of size (%d, %d)" % (n, B))
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    if any(k not in WRT for k in wrt):
        raise ValueError("%s: wrt names %s; it takes 'P', 'q', 'G', 'h', 'A', 'b'" % (who, ", ".join(repr(k) for k in wrt if k not in WRT)))
    gv = np.ascontiguousarray(g.T).reshape(-1)
    sP, sG, sA = data[0][1], data[2][1], data[4][1]
    L = _lib.lib()
    ux, uy, uz = (np.zeros((rows, B), order="F") for rows in (n, p, N))
    gexit, steps, cen = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.zeros(B)
    mats = {}
    for k, rows, stride in (("P", n, sP), ("G", N, sG), ("A", p, sA)):
        mats[k] = np.zeros((B if stride else 1) * rows * n) if k in wrt and rows else None
    args, keep = _common(sizes, data, vecs, code, opts)
    args += [_lib.pd(gv), _lib.pd(ux), _lib.pd(uy) if p else None, _lib.pd(uz)]
    args += [None if mats[k] is None else _lib.pd(mats[k]) for k in ("P", "G", "A")] + [_lib.pd(cen), _lib.pi(steps), _lib.pi(gexit)]
    _lib.raise_for(L.kvx_coneqp_batch_vjp(*args), "kvx_coneqp_batch_vjp")
    del keep
    out = {"ux": ux, "uy": uy, "uz": uz, "exit": gexit, "centrality": cen, "centering steps": steps}
    done = gexit == EXIT_DONE
    for k in wrt:
        if k == "q":
            out[k] = ux.copy()
        elif k == "h":
            out[k] = _column_gradient(0.0 - uz, h, data[3][1] == 0, done)            # 0 - u: no negative zeros
        elif k == "b":
            out[k] = _column_gradient(0.0 - uy, b, data[5][1] == 0, done) if p else None
        else:
            rows, stride = {"P": (n, sP), "G": (N, sG), "A": (p, sA)}[k]
            out[k] = None if mats[k] is None else _from_members(mats[k], stride == 0, rows, n, B)
    return out


def _perturbation(name, v, like, n, B, rows):
    """(values or None, member stride) of one perturbation, checked as coneqp_batch checks the datum it perturbs."""
    if v is None:
        return None, 0
    if like in ("P", "G", "A"):
        vals, stride, _ = qpbatch._matrix(v, name, n, B, rows=rows)
        return vals, stride
    return qpbatch._shared_or_batch(v, name, rows, B, "'%s' must be a 'd' matrix of size (%d,1)" % (name, rows))


def coneqp_batch_jvp(P, q, G, h, dims, A=None, b=None, *, sol, dP=None, dq=None, dG=None, dh=None, dA=None, db=None, options=None):
    who = "coneqp_batch_jvp"
    opts = _options(who, options)
    sizes, data = _problem(who, P, q, G, h, dims, A, b)
    B, n, ml, qd, sd, N, p = sizes
    vecs, code = _solution(sol, B, n, N, p)
    pert = [_perturbation("d" + k, v, k, n, B, rows)
            for k, v, rows in (("P", dP, n), ("q", dq, n), ("G", dG, N), ("h", dh, N), ("A", dA, p), ("b", db, p))]
    L = _lib.lib()
    dx, dy, dz, ds = (np.zeros((rows, B), order="F") for rows in (n, p, N, N))
    gexit, steps, cen = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.zeros(B)
    args, keep = _common(sizes, data, vecs, code, opts)
    for k, (vals, stride) in zip(WRT, pert):
        args += [None if vals is None or (k in "Ab" and not p) else _lib.pd(vals), stride]
    args += [_lib.pd(dx), _lib.pd(dy) if p else None, _lib.pd(dz), _lib.pd(ds), _lib.pd(cen), _lib.pi(steps), _lib.pi(gexit)]
    _lib.raise_for(L.kvx_coneqp_batch_jvp(*args), "kvx_coneqp_batch_jvp")
    del keep
    return {"x": dx, "y": dy, "z": dz, "s": ds, "exit": gexit, "centrality": cen, "centering steps": steps}
