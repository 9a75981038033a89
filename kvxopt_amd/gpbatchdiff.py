"""Derivatives of a solved batch of small dense geometric programs:

    gp_batch_vjp(K, F, g, G=None, h=None, A=None, b=None, *, sol, gx, wrt=("F", "g", "G", "h", "A", "b"), options=None) -> dict
    gp_batch_jvp(K, F, g, G=None, h=None, A=None, b=None, *, sol, dF=None, dg=None, dG=None, dh=None, dA=None, db=None,
                 options=None) -> dict

also kvxopt_amd.solvers.gp_batch_vjp / gp_batch_jvp.  `sol` is what gp_batch returned for the same problem arguments; its 'x', 'y',
'znl', 'snl', 'zl', 'sl' and 'exit' are read.  Write zeta_0 = 1 and zeta_i = znl_i, and per block i (block 0 is the objective)
y_i = softmax(F_i x + g_i), Df_i = y_i'F_i.  At the returned point of member b the differentiated optimality conditions are a
linear system in x -- of order n: gp_batch dropped the epigraph row, whose dual tends to 1 -- with the matrix

    K = [ H  A'  J' ;  A  0  0 ;  J  0  -diag(s / z) ],     H = sum_{i >= 0} zeta_i F_i'(diag y_i - y_i y_i')F_i,
                                                            J = [Df_1 .. Df_mnl; G],  s = (snl, sl),  z = (znl, zl).

Its reduced matrix H + J' diag(z / s) J is the Schur complement on t of the matrix gp_batch factors at every iteration, and is
assembled from the same staged rows, so a derivative costs about one interior-point iteration per member
(csrc/gp_batch_diff.hip: one workgroup per member, one launch; kvx_gp_batch_vjp / kvx_gp_batch_jvp).  The rows are an orthant, so
diag(s / z) linearises complementarity exactly at any point and no centring pass is needed.  The mathematics is that of Amos &
Kolter, "OptNet" (2017), section 3; what a QP does not have is that the data enter through the softmax weights.

  reverse  given gx = dl/dx (n x B), K [ux; uy; uz] = [-gx; 0; 0] with uz = (uznl, uzl) and uznl_0 := 0 for the objective block;
           with e_k = (F_k - Df_i) ux for term k of block i,
               dl/dg_k = y_k (zeta_i e_k + uznl_i),    dl/dF_k = zeta_i y_k ux' + (dl/dg_k) x',
               dl/dG = uzl x' + zl ux',  dl/dh = -uzl,  dl/dA = uy x' + y ux',  dl/db = -uy.
           The result has 'ux' (n x B), 'uy' (p x B), 'uznl' (mnl x B), 'uzl' (ml x B), 'exit' (B) and for each name in `wrt` the
           gradient in the shape the argument was given: a (B, rows, n) matrix argument gets a (B, rows, n) gradient, columns
           get columns; a matrix all members share, or a shared column h or b, gets the SUM over the done members as one item.
           g has one column per member, so its gradient is l x B.  Matrix gradients not named in `wrt` are not formed on the
           device.  With ml = 0 the gradients of G and h are None, with p = 0 those of A and b.
  forward  given perturbations dF, dg, dG, dh, dA, db -- each None (zero), one item shared by all members, or per member, in the
           shapes gp_batch accepts for F .. b; dg is l x B or one column -- with v = dF x + dg,
               bx = -(sum_i zeta_i [dF_i'y_i + F_i'(y_i o v_i - y_i (y_i'v_i))] + dG'zl + dA'y),   by = db - dA x,
               bz = (-y_i'v_i for i >= 1;  dh - dG x),       K [dx; dy; dz] = [bx; by; bz],        ds = -(s / z) o dz.
           The result has 'x', 'y', 'znl', 'snl', 'zl', 'sl' (the directional derivatives, shaped as in `sol`) and 'exit'.
  exit     0 done; 1 skipped because the member's sol['exit'] is not 0; 2 a pivot failed or some s_k, z_k is not positive and
           finite.  A member with 1 or 2 has zeros in every output and adds nothing to a shared sum; the others are undisturbed.
  options  only 'refinement': 0 to 3 steps of iterative refinement on the full system, default 1 (DESIGN section 22 has the
           table that decides it).  K is not differentiable.

The truncation remark of qp_batch_vjp holds here too: the derivative is that of the point handed in, a point of the central path
and not the exact optimum, so solve with tolerances near 1e-8 to 1e-9 where derivatives are wanted.

The limits and the texts of the argument checks are those of gp_batch.  Every check runs before a device is asked for; there is
no CPU fallback.  Not carried: several cotangents per call, gradients with respect to y and z, the derivative fused into the
forward launch, a torch.autograd.Function."""
import numpy as np

from . import _batch, _batchdiff, _lib, gpbatch
from ._batchdiff import EXIT_DONE, EXIT_FAILED, EXIT_SKIPPED, MAX_REFINEMENT  # noqa: F401

WRT = ("F", "g", "G", "h", "A", "b")
DEFAULT_REFINEMENT = 1


def _refinement(who, options):
    o = dict(options or {})
    ref = o.pop("refinement", DEFAULT_REFINEMENT)
    if o:
        raise ValueError("%s: options accepts only 'refinement', not %s" % (who, ", ".join(repr(k) for k in sorted(o, key=str))))
    return _batchdiff.count(who, "refinement", ref, MAX_REFINEMENT)


def _front(who, K, F, g, G, h, A, b, sol, options):
    """Everything both entries check first.  Returns the sizes, the data of gp_batch._prepare, the solution with s and z as the C
    entries take them (N = mnl + 1 + ml rows per member, the objective row first and not read) and common(), the leading
    arguments of all four C entries."""
    ref = _refinement(who, options)
    (B, n, K, ml, p), data = _batchdiff.problem(who, "gp_batch", gpbatch._prepare, K, F, g, G, h, A, b)
    m, l = len(K), sum(K)
    keys = (("x", n), ("y", p), ("znl", m - 1), ("snl", m - 1), ("zl", ml), ("sl", ml))
    (x, y, znl, snl, zl, sl), code = _batchdiff.solution(sol, "gp_batch", B, n, ml, p, keys=keys)
    s, z = np.zeros((B, m + ml)), np.zeros((B, m + ml))
    s[:, 1:m], s[:, m:], z[:, 1:m], z[:, m:] = snl.reshape(B, m - 1), sl.reshape(B, ml), znl.reshape(B, m - 1), zl.reshape(B, ml)
    s, z = s.reshape(-1), z.reshape(-1)
    (Fv, sF), (gv, sg), (Gv, sG), _, (Av, sA), _ = data
    Kp = _batch.orders(K)[1]

    def common():
        return [B, n, m - 1, Kp, ml, p, _lib.pd(Fv), sF, _lib.pd(gv), sg, _lib.pd(Gv) if ml else None, sG, _lib.pd(Av) if p else None, sA,
                _lib.pd(x), _lib.pd(y) if p else None, _lib.pd(s), _lib.pd(z), _lib.pi(code), ref]
    return (B, n, m, l, ml, p), data, common


def gp_batch_vjp(K, F, g, G=None, h=None, A=None, b=None, *, sol, gx, wrt=WRT, options=None):
    who = "gp_batch_vjp"
    (B, n, m, l, ml, p), data, common = _front(who, K, F, g, G, h, A, b, sol, options)
    gv = _batchdiff.cotangent(gx, n, B)
    wrt = _batchdiff.named(who, wrt, WRT)
    (_, sF), _, (_, sG), (_, sh), (_, sA), (_, sb) = data
    ux, uy, uz, gg = (np.zeros((r, B), order="F") for r in (n, p, m + ml, l))
    gexit = np.zeros(B, dtype=np.int64)
    shapes = {"F": (l, sF), "G": (ml, sG), "A": (p, sA)}
    mats = {k: np.zeros((B if stride else 1) * r * n) if k in wrt and r else None for k, (r, stride) in shapes.items()}
    args = common() + [_lib.pd(gv), _lib.pd(ux), _lib.pd(uy) if p else None, _lib.pd(uz), _lib.pd(gg)]
    args += [None if mats[k] is None else _lib.pd(mats[k]) for k in ("F", "G", "A")] + [_lib.pi(gexit)]
    _lib.raise_for(_lib.lib().kvx_gp_batch_vjp(*args), "kvx_gp_batch_vjp")
    uznl, uzl = np.asfortranarray(uz[1:m]), np.asfortranarray(uz[m:])
    out = {"ux": ux, "uy": uy, "uznl": uznl, "uzl": uzl, "exit": gexit}
    done = gexit == EXIT_DONE
    for k in wrt:
        if k == "g":
            out[k] = gg
        elif k == "h":
            out[k] = _batchdiff.column_gradient(0.0 - uzl, h, sh == 0, done) if ml else None      # 0 - u: no negative zeros
        elif k == "b":
            out[k] = _batchdiff.column_gradient(0.0 - uy, b, sb == 0, done) if p else None
        else:
            r, stride = shapes[k]
            out[k] = None if mats[k] is None else _batchdiff.from_members(mats[k], stride == 0, r, n, B)
    return out


def gp_batch_jvp(K, F, g, G=None, h=None, A=None, b=None, *, sol, dF=None, dg=None, dG=None, dh=None, dA=None, db=None, options=None):
    who = "gp_batch_jvp"
    (B, n, m, l, ml, p), _, common = _front(who, K, F, g, G, h, A, b, sol, options)
    sizes = (l, l, ml, ml, p, p)
    pert = _batchdiff.perturbations((dF, dg, dG, dh, dA, db), B, n, ml, p, names=WRT, sizes=sizes, defines="g")
    dx, dy, dz, ds = (np.zeros((r, B), order="F") for r in (n, p, m + ml, m + ml))
    gexit = np.zeros(B, dtype=np.int64)
    args = common()
    for (vals, stride), r in zip(pert, sizes):
        args += [None if vals is None or not r else _lib.pd(vals), stride]
    args += [_lib.pd(dx), _lib.pd(dy) if p else None, _lib.pd(dz), _lib.pd(ds), _lib.pi(gexit)]
    _lib.raise_for(_lib.lib().kvx_gp_batch_jvp(*args), "kvx_gp_batch_jvp")
    return {"x": dx, "y": dy, "znl": np.asfortranarray(dz[1:m]), "snl": np.asfortranarray(ds[1:m]), "zl": np.asfortranarray(dz[m:]),
            "sl": np.asfortranarray(ds[m:]), "exit": gexit}
