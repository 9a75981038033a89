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
no CPU fallback.  Not carried: several cotangents per call, derivatives of lp_batch (coneqp_batch: coneqpbatchdiff, gp_batch: gpbatchdiff), gradients with
respect to y and z, the derivative fused into the forward launch, a torch.autograd.Function."""
from . import _batchdiff, _lib, qpbatch
from ._batchdiff import EXIT_DONE, EXIT_FAILED, EXIT_SKIPPED, MAX_REFINEMENT, WRT  # noqa: F401


def _refinement(who, options):
    o = dict(options or {})
    ref = o.pop("refinement", 1)
    if o:
        raise ValueError("%s: options accepts only 'refinement', not %s" % (who, ", ".join(repr(k) for k in sorted(o, key=str))))
    return _batchdiff.count(who, "refinement", ref, MAX_REFINEMENT)


def _problem(who, P, q, G, h, A, b):
    """qp_batch's own checks of the problem arguments, under the entry's name."""
    return _batchdiff.problem(who, "qp_batch", qpbatch._prepare, P, q, G, h, A, b)


def _common(dims, data, vecs, code, ref):
    """The leading arguments of all four C entries: sizes, P, G, A with strides, the solution, the refinement."""
    (Pv, sP), _, (Gv, sG), _, (Av, sA), _ = data
    p = dims[3]
    return list(dims) + [_lib.pd(Pv), sP, _lib.pd(Gv), sG, _lib.pd(Av) if p else None, sA] + _batchdiff.solution_pointers(vecs, code, p) + [ref]


def qp_batch_vjp(P, q, G, h, A=None, b=None, *, sol, gx, wrt=WRT, options=None):
    who = "qp_batch_vjp"
    ref = _refinement(who, options)
    dims, data = _problem(who, P, q, G, h, A, b)
    B, n, ml, p = dims
    vecs, code = _batchdiff.solution(sol, "qp_batch", B, n, ml, p)
    return _batchdiff.vjp("kvx_qp_batch_vjp", who, lambda: _common(dims, data, vecs, code, ref), _batchdiff.strides(data), B, n, ml, p, gx, wrt, h, b)


def qp_batch_jvp(P, q, G, h, A=None, b=None, *, sol, dP=None, dq=None, dG=None, dh=None, dA=None, db=None, options=None):
    who = "qp_batch_jvp"
    ref = _refinement(who, options)
    dims, data = _problem(who, P, q, G, h, A, b)
    B, n, ml, p = dims
    vecs, code = _batchdiff.solution(sol, "qp_batch", B, n, ml, p)
    pert = _batchdiff.perturbations((dP, dq, dG, dh, dA, db), B, n, ml, p)
    return _batchdiff.jvp("kvx_qp_batch_jvp", lambda: _common(dims, data, vecs, code, ref), pert, B, n, ml, p)
