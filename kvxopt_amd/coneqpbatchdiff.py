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

from . import _batch, _batchdiff, coneqpbatch
from ._batchdiff import EXIT_DONE, EXIT_FAILED, EXIT_SKIPPED, MAX_REFINEMENT, WRT  # noqa: F401

EXIT_NOT_CENTRED = 3
MAX_CENTERING = 16
DEFAULT_CENTERING, DEFAULT_CENTOL = 8, 1e-6               # DESIGN 21 has the table they are chosen from


def _options(who, options):
    o = dict(options or {})
    ref, cen, tol = o.pop("refinement", 1), o.pop("centering", DEFAULT_CENTERING), o.pop("centol", DEFAULT_CENTOL)
    if o:
        raise ValueError("%s: options accepts only 'refinement', 'centering' and 'centol', not %s"
                         % (who, ", ".join(repr(k) for k in sorted(o, key=str))))
    ref, cen = _batchdiff.count(who, "refinement", ref, MAX_REFINEMENT), _batchdiff.count(who, "centering", cen, MAX_CENTERING)
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol > 0:
        raise ValueError("options['centol'] must be a positive scalar")
    return ref, cen, float(tol)


def _problem(who, P, q, G, h, dims, A, b):
    """coneqp_batch's own checks of the problem arguments, under the entry's name."""
    return _batchdiff.problem(who, "coneqp_batch", coneqpbatch._prepare, P, q, G, h, dims, A, b)


def _common(sizes, data, vecs, code, opts):
    """The leading arguments of all four C entries: sizes, the cone, the data with strides, the solution, the options."""
    B, n, ml, qd, sd, N, p = sizes
    head = [B, n, ml] + _batch.orders(qd) + _batch.orders(sd) + [p]
    return head + _batch.pointers(data) + _batchdiff.solution_pointers(vecs, code, p) + list(opts)


def _extra(B):
    """The results the cone entries have beyond the orthant's, in the order of the C entries."""
    return {"centrality": np.zeros(B), "centering steps": np.zeros(B, dtype=np.int64)}


def coneqp_batch_vjp(P, q, G, h, dims, A=None, b=None, *, sol, gx, wrt=WRT, options=None):
    who = "coneqp_batch_vjp"
    opts = _options(who, options)
    sizes, data = _problem(who, P, q, G, h, dims, A, b)
    B, n, ml, qd, sd, N, p = sizes
    vecs, code = _batchdiff.solution(sol, "coneqp_batch", B, n, N, p, copy=True)
    return _batchdiff.vjp("kvx_coneqp_batch_vjp", who, lambda: _common(sizes, data, vecs, code, opts),
                          _batchdiff.strides(data), B, n, N, p, gx, wrt, h, b, _extra(B))


def coneqp_batch_jvp(P, q, G, h, dims, A=None, b=None, *, sol, dP=None, dq=None, dG=None, dh=None, dA=None, db=None, options=None):
    who = "coneqp_batch_jvp"
    opts = _options(who, options)
    sizes, data = _problem(who, P, q, G, h, dims, A, b)
    B, n, ml, qd, sd, N, p = sizes
    vecs, code = _batchdiff.solution(sol, "coneqp_batch", B, n, N, p, copy=True)
    pert = _batchdiff.perturbations((dP, dq, dG, dh, dA, db), B, n, N, p)
    return _batchdiff.jvp("kvx_coneqp_batch_jvp", lambda: _common(sizes, data, vecs, code, opts), pert, B, n, N, p, _extra(B))
