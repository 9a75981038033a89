"""The 'q' and 's' cone kernels (csrc/kkt_q.hip, csrc/kkt_s.hip) at orders that use the whole 256-thread workgroup: past one
wavefront (63 / 64 / 65), past one pass of the stride loops (255 / 256 / 257, m * m = 256 / 289), several passes (513, 1000),
a second pass over the column pairs of the Jacobi sweeps (9 / 10) and row loops beyond 64 lanes (65, 90).  Everything goes
through the host-array wrappers of kvxopt_amd.misc; the reference is oracle/kvx_oracle.py (pinned on the goldens G15 / G16 by
tests/test_oracle.py) evaluated in np.longdouble on the float64 inputs the device gets.

Tolerances.  'q' cones: 1e-13 of the infinity norm of the long-double vector of the cone, 1e-13 of max(1, |value|) for
scalars (the tolerance of test_second_order_cone_scaling_golden); sdot relative to sum |x_i y_i|.  The float64 oracle itself
differs from the long-double one by at most 7.4e-15 with this generator (margin 0.05, orders up to 4099, five seeds, both
layouts; the worst is sinv, then update_scaling's z / b at 4.3e-15 and max_step at 4.2e-15), a third of a quarter of the
bound.  's' blocks: 1e-12 of the largest entry of the block for the entrywise operations, 1e-12 for lambda against numpy's
singular values, 1e-11 for the products and identities of update_scaling (the tolerances of the G16 test); storage helpers
bit for bit.

Worst device error / bound per operation measured on an MI355X (both layouts, every cone or block, every column; the module
prints the table at its end under -s):
  'q'  compute_scaling  v 0.0045   lmbda 0.0028   beta 0.0067
       scale            N 0.0063   I 0.0031       scale then inverse (bound 1e-12) 0.00077
       scale2           N 0.015    I 0.0019
       sprod 0.0036     sinv 0.022     ssqr 0.0031     sdot 0.0023     max_step 0.019
       update_scaling   s 0.017    z 0.017    lmbda 0.0055    v 0.0029    beta 0.016
       the 'l' entries in front of the cones, any operation: at most 0.00095
  's'  update_scaling   lmbda 0.011   r r' 0.00073   rti rti' 0.00070   rti' r = I 0.00046   U' U = I 0.00021
                        V' V = I 0.0022   U diag(lmbda) V' = Lz' Ls 0.0015
       scale            NN 0.00068   TN 0.00075   NI 0.00078   TI 0.00087
       scale2 0.00022   sprod 0.0010   sprod 'D' 0.000077   sinv 0.000069   ssqr 0.000056   sdot 0.00014
  conelp  'q' order 300: x 0.014, objective 0.065     's' order 65: t 0.0050
"""
import functools
import types

import numpy as np
import pytest

from kvxopt_amd import _lib, misc, solvers
from kvxopt_amd.base import matrix
from oracle import kvx_oracle as orc

pytestmark = pytest.mark.gpu

LD = np.longdouble
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()
    yield
    print()
    for op in sorted(_WORST):
        print("worst error / bound  %-42s %.3g" % (op, _WORST[op]))


def _within(op, got, want, tol, scale=None):
    """max |got - want| <= tol * scale (default: the largest |entry| of want); records error / bound before it asserts."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    assert got.shape == want.shape, (op, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    bound = tol * float(np.max(np.abs(want)) if scale is None else scale)
    _WORST[op] = max(_WORST.get(op, 0.0), err / bound)
    assert err <= bound, (op, err, bound)


def _scalar(op, got, want, tol):
    _within(op, got, want, tol, scale=max(1.0, abs(float(want))))


def _twice(run):
    """The outputs of run(), after a second run gave the same bytes (the kernels sum in a fixed order)."""
    a, b = run(), run()
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    return a


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


# ---- 'q' cones -------------------------------------------------------------------------------------------------------------
QL, Q = 5, [1, 2, 3, 63, 64, 65, 255, 256, 257, 513, 1000]
MARGIN = 0.05


def interior_q(rng, k, q=Q, ml=QL, margin=MARGIN):
    """A point in the interior of the cone: head = |u| (1 + margin (0.5 + U(0, 1))) over a tail u ~ N(0, 1); the cone of order
    1 takes its head from (0.5, 1.5)."""
    x = rng.uniform(0.3, 2.0, k + ml + sum(q))
    ind = k + ml
    for m in q:
        if m == 1:
            x[ind] = rng.uniform(0.5, 1.5)
        else:
            u = rng.standard_normal(m - 1)
            x[ind + 1:ind + m] = u
            x[ind] = np.linalg.norm(u) * (1.0 + margin * (0.5 + rng.uniform()))
        ind += m
    return x


def _q_stage1(s, z, nl, q, T):
    """compute_scaling of every cone in the number type T: lists of v, beta, lmbda."""
    out, o = [], nl
    for m in q:
        out.append(orc.compute_scaling_q(s[o:o + m].astype(T), z[o:o + m].astype(T)))
        o += m
    return [c[0] for c in out], [c[1] for c in out], [c[2] for c in out]


def q_reference(C, T):
    """Every 'q' operation of this module, cone by cone, in the number type T on the float64 inputs of the case C."""
    R = types.SimpleNamespace(scale={"N": [], "I": []}, scale2={"N": [], "I": []}, sprod=[], sinv=[], ssqr=[], sdot=[],
                              sabs=[], max_step=[], us=[])
    R.v, R.beta, R.lm = _q_stage1(C.s, C.z, C.nl, C.q, T)
    o = C.nl
    for i, m in enumerate(C.q):
        sl = slice(o, o + m)
        v, beta, lm = C.v64[i].astype(T), T(C.beta64[i]), C.lm64[sl].astype(T)
        x1, y1 = C.x1[sl].astype(T), C.y1[sl].astype(T)
        for inv in "NI":
            R.scale[inv].append(np.column_stack([orc.scale_q(C.X[sl, c].astype(T), v, beta, inv) for c in range(C.X.shape[1])]))
            R.scale2[inv].append(orc.scale2_q(lm, x1, inv))
        R.sprod.append(orc.sprod_q(x1, y1))
        R.sinv.append(orc.sinv_q(x1, y1))
        R.ssqr.append(orc.ssqr_q(y1))
        R.sdot.append(np.dot(x1, y1))
        R.sabs.append(np.sum(np.abs(x1 * y1)))
        R.max_step.append(orc.max_step_q(x1))
        R.us.append(orc.update_scaling_q(v, beta, C.s2[sl].astype(T), C.z2[sl].astype(T)))
        o += m
    return R


def make_q_case(mnl, seed, q=Q, margin=MARGIN):
    """Inputs (float64) of one layout: interior points s, z (compute_scaling), x1, y1 (the products), s2, z2 (update_scaling), a
    3-column matrix X with two padding rows, and v, beta, lmbda of compute_scaling rounded from long double (what scale,
    scale2 and update_scaling start from)."""
    k = mnl or 0
    rng = np.random.default_rng(seed)
    C = types.SimpleNamespace(mnl=mnl, k=k, q=list(q), nl=k + QL, N=k + QL + sum(q), dims={"l": QL, "q": list(q), "s": []})
    C.s, C.z, C.x1, C.y1, C.s2, C.z2 = (interior_q(rng, k, q, QL, margin) for _ in range(6))
    C.X = rng.standard_normal((C.N + 2, 3))
    v, beta, lm = _q_stage1(C.s, C.z, C.nl, C.q, LD)
    C.v64 = [np.asarray(a, dtype=np.float64) for a in v]
    C.beta64 = [float(b) for b in beta]
    C.lm64 = np.concatenate([np.sqrt(C.s[:C.nl] * C.z[:C.nl])] + [np.asarray(a, dtype=np.float64) for a in lm])
    return C


@functools.lru_cache(maxsize=None)
def q_case(mnl):
    C = make_q_case(mnl, 2500 + (mnl or 0))
    C.ref = q_reference(C, LD)
    return C


def _cones(C):
    o = C.nl
    for i, m in enumerate(C.q):
        yield i, slice(o, o + m), m
        o += m


def _W_q(C):
    """W with the oracle's v, beta and d = di = 1 exactly, so that scale leaves the 'l' rows bit for bit."""
    W = {"d": matrix(np.ones(QL)), "di": matrix(np.ones(QL)), "v": [matrix(v.copy()) for v in C.v64], "beta": list(C.beta64),
         "r": [], "rti": []}
    if C.mnl:
        W["dnl"], W["dnli"] = matrix(np.ones(C.k)), matrix(np.ones(C.k))
    return W


QTOL = 1e-13
MNL_Q = [None, 3]


@pytest.mark.parametrize("mnl", MNL_Q)
def test_q_compute_scaling(mnl):
    C = q_case(mnl)

    def run():
        lm = matrix(0.0, (C.N, 1))
        W = misc.compute_scaling(matrix(C.s), matrix(C.z), lm, C.dims, C.mnl)
        return [lm._a.copy(), np.array(W["beta"])] + [v._a.copy() for v in W["v"]]
    out = _twice(run)
    lm, beta, vs = out[0], out[1], out[2:]
    assert [v.size for v in vs] == C.q
    _within("q compute_scaling lmbda 'l'", lm[:C.nl], np.sqrt(_ld(C.s[:C.nl]) * _ld(C.z[:C.nl])), QTOL)
    for i, sl, m in _cones(C):
        _within("q compute_scaling v", vs[i], C.ref.v[i], QTOL)
        _within("q compute_scaling lmbda", lm[sl], C.ref.lm[i], QTOL)
        _scalar("q compute_scaling beta", beta[i], C.ref.beta[i], QTOL)


@pytest.mark.parametrize("mnl", MNL_Q)
def test_q_scale_all_forms_on_three_padded_columns(mnl):
    C = q_case(mnl)
    W = _W_q(C)
    for tr in "NT":
        for inv in "NI":
            def run():
                x = matrix(C.X.copy(order="F"))
                misc.scale(x, W, trans=tr, inverse=inv)
                return [x.a.copy()]
            got = _twice(run)[0]
            for i, sl, m in _cones(C):
                for c in range(3):
                    _within("q scale " + inv, got[sl, c], C.ref.scale[inv][i][:, c], QTOL)
            assert got[:C.nl].tobytes() == C.X[:C.nl].tobytes() and got[C.N:].tobytes() == C.X[C.N:].tobytes(), (tr, inv)
    x = matrix(C.X.copy(order="F"))
    misc.scale(x, W)
    misc.scale(x, W, inverse="I")
    _within("q scale then inverse", x.a, C.X, 1e-12)
    assert x.a[:C.nl].tobytes() == C.X[:C.nl].tobytes() and x.a[C.N:].tobytes() == C.X[C.N:].tobytes()


@pytest.mark.parametrize("mnl", MNL_Q)
def test_q_scale2_sprod_sinv_ssqr(mnl):
    C = q_case(mnl)
    nl, x1, y1 = C.nl, C.x1, C.y1
    ops = {"scale2 N": (lambda a: misc.scale2(matrix(C.lm64), a, C.dims, C.k), C.ref.scale2["N"], _ld(x1[:nl]) / _ld(C.lm64[:nl])),
           "scale2 I": (lambda a: misc.scale2(matrix(C.lm64), a, C.dims, C.k, inverse="I"), C.ref.scale2["I"],
                        _ld(x1[:nl]) * _ld(C.lm64[:nl])),
           "sprod": (lambda a: misc.sprod(a, matrix(y1), C.dims, C.k), C.ref.sprod, _ld(x1[:nl]) * _ld(y1[:nl])),
           "sinv": (lambda a: misc.sinv(a, matrix(y1), C.dims, C.k), C.ref.sinv, _ld(x1[:nl]) / _ld(y1[:nl])),
           "ssqr": (lambda a: misc.ssqr(a, matrix(y1), C.dims, C.k), C.ref.ssqr, _ld(y1[:nl]) * _ld(y1[:nl]))}
    for name, (fn, ref, ref_l) in ops.items():
        def run():
            a = matrix(0.0, (C.N, 1)) if name == "ssqr" else matrix(x1.copy())
            fn(a)
            return [a._a.copy()]
        got = _twice(run)[0]
        _within("q %s 'l'" % name, got[:nl], ref_l, QTOL)
        for i, sl, m in _cones(C):
            _within("q " + name, got[sl], ref[i], QTOL)


@pytest.mark.parametrize("mnl", MNL_Q)
def test_q_sdot_and_max_step_cone_by_cone(mnl):
    C = q_case(mnl)
    nl, x1, y1 = C.nl, C.x1, C.y1
    dot_l, abs_l = np.dot(_ld(x1[:nl]), _ld(y1[:nl])), float(np.sum(np.abs(x1[:nl] * y1[:nl])))
    got = _twice(lambda: [np.array(misc.sdot(matrix(x1), matrix(y1), C.dims, C.k))])[0]
    _within("q sdot", got, dot_l + sum(C.ref.sdot), QTOL, scale=abs_l + float(sum(C.ref.sabs)))
    got = _twice(lambda: [np.array(misc.max_step(matrix(x1), C.dims, C.k))])[0]
    _scalar("q max_step", got, max([np.max(-_ld(x1[:nl]))] + C.ref.max_step), QTOL)
    # one cone at a time: the other cones hold zeros (sdot) or points far inside (max_step)
    far = np.zeros(C.N)
    far[:nl] = 1e6
    for i, sl, m in _cones(C):
        far[sl.start] = 1e6
    for i, sl, m in _cones(C):
        xm = np.zeros(C.N)
        xm[sl] = x1[sl]
        _within("q sdot", misc.sdot(matrix(xm), matrix(y1), C.dims, C.k), C.ref.sdot[i], QTOL, scale=float(C.ref.sabs[i]))
        xm = far.copy()
        xm[sl] = x1[sl]
        _scalar("q max_step", misc.max_step(matrix(xm), C.dims, C.k), C.ref.max_step[i], QTOL)


@pytest.mark.parametrize("mnl", MNL_Q)
def test_q_update_scaling_in_place(mnl):
    C = q_case(mnl)
    nl = C.nl

    def run():
        W = _W_q(C)
        lm, ms, mz = matrix(C.lm64.copy()), matrix(C.s2.copy()), matrix(C.z2.copy())
        misc.update_scaling(W, lm, ms, mz)
        return [ms._a.copy(), mz._a.copy(), lm._a.copy(), np.array(W["beta"])] + [v._a.copy() for v in W["v"]]
    out = _twice(run)
    s, z, lm, beta, vs = out[0], out[1], out[2], out[3], out[4:]
    _within("q update_scaling lmbda 'l'", lm[:nl], np.sqrt(_ld(C.s2[:nl])) * np.sqrt(_ld(C.z2[:nl])), QTOL)
    for i, sl, m in _cones(C):
        rs, rz, rv, rbeta, rlm = C.ref.us[i]
        _within("q update_scaling s", s[sl], rs, QTOL)
        _within("q update_scaling z", z[sl], rz, QTOL)
        _within("q update_scaling lmbda", lm[sl], rlm, QTOL)
        _within("q update_scaling v", vs[i], rv, QTOL)
        _scalar("q update_scaling beta", beta[i], rbeta, QTOL)


# ---- 's' blocks ------------------------------------------------------------------------------------------------------------
SL, SQ, SD = 2, [3], [1, 2, 9, 10, 16, 17, 33, 64, 65, 90]
MNL_S = [None, 2]


def _sblocks(vec, off, sd=SD):
    out, o = [], off
    for m in sd:
        out.append(vec[o:o + m * m].reshape((m, m), order="F"))
        o += m * m
    return out


@functools.lru_cache(maxsize=None)
def s_case(mnl):
    """Inputs of one layout: two pairs of interior points (blocks B B' / m + diag(U(0.2, 1.5))), x1 (blocks not symmetric: only
    the lower triangles are read), y1, a lmbda / diagonal y in the cdim_diag layout and a 3-column matrix with three padding rows."""
    k = mnl or 0
    rng = np.random.default_rng(3500 + k)
    nlq = k + SL + sum(SQ)
    C = types.SimpleNamespace(mnl=mnl, k=k, nlq=nlq, tot2=sum(m * m for m in SD), tot1=sum(SD), dims={"l": SL, "q": list(SQ), "s": list(SD)})
    C.N, C.Nd, C.Np = nlq + C.tot2, nlq + C.tot1, nlq + sum(m * (m + 1) // 2 for m in SD)

    def interior(diag=False):
        parts = [rng.uniform(0.3, 2.0, k + SL)]
        for m in SQ:
            u = rng.standard_normal(m - 1)
            parts.append(np.concatenate([[np.linalg.norm(u) + rng.uniform(0.2, 1.5)], u]))
        for m in SD:
            if diag:
                parts.append(rng.uniform(0.4, 2.0, m))
            else:
                B = rng.standard_normal((m, m))
                parts.append((B @ B.T / m + np.diag(rng.uniform(0.2, 1.5, m))).reshape(-1, order="F"))
        return np.concatenate(parts)
    C.s, C.z, C.s2, C.z2 = interior(), interior(), interior(), interior()
    C.x1 = interior() * 0.7 + 0.1 * rng.standard_normal(C.N)
    C.y1 = interior()
    C.lmd, C.yd = interior(diag=True), interior(diag=True)
    C.X = rng.standard_normal((C.N + 3, 3))
    return C


@functools.lru_cache(maxsize=None)
def _s_scaling(mnl):
    """The device's own W of the first pair of points (the host dictionary; copied before use)."""
    C = s_case(mnl)
    lm = matrix(0.0, (C.Nd, 1))
    return misc.compute_scaling(matrix(C.s), matrix(C.z), lm, C.dims, C.mnl)


def _copy_W(W):
    return {key: ([matrix(b) if isinstance(b, matrix) else b for b in val] if isinstance(val, list) else matrix(val)) for key, val in W.items()}


@pytest.mark.parametrize("mnl", MNL_S)
def test_s_update_scaling_with_accumulated_v(mnl):
    C = s_case(mnl)
    W0 = _s_scaling(mnl)
    s_in, z_in = C.s2.copy(), C.z2.copy()
    Ls = [np.linalg.cholesky(B) for B in _sblocks(C.s2, C.nlq)]
    Lz = [np.linalg.cholesky(B) for B in _sblocks(C.z2, C.nlq)]
    s_in[C.nlq:] = np.concatenate([L.reshape(-1, order="F") for L in Ls])
    z_in[C.nlq:] = np.concatenate([L.reshape(-1, order="F") for L in Lz])

    def run():
        W = _copy_W(W0)
        lm, ms, mz = matrix(0.0, (C.Nd, 1)), matrix(s_in.copy()), matrix(z_in.copy())
        misc.update_scaling(W, lm, ms, mz)
        return [lm._a.copy(), ms._a.copy(), mz._a.copy()] + [r._a.copy() for r in W["r"]] + [r._a.copy() for r in W["rti"]]
    out = _twice(run)
    lm, U, Vt = out[0], _sblocks(out[1], C.nlq), _sblocks(out[2], C.nlq)
    ns = len(SD)
    il = C.nlq
    for i, m in enumerate(SD):
        R, T = out[3 + i].reshape((m, m), order="F"), out[3 + ns + i].reshape((m, m), order="F")
        M = Lz[i].T @ Ls[i]
        lmk = lm[il:il + m]
        _within("s update_scaling lmbda", lmk, np.linalg.svd(M, compute_uv=False), 1e-12)
        r2, t2, _ = orc.update_scaling_s(W0["r"][i].a, W0["rti"][i].a, Ls[i], Lz[i])
        _within("s update_scaling r r'", R @ R.T, r2 @ r2.T, 1e-11)
        _within("s update_scaling rti rti'", T @ T.T, t2 @ t2.T, 1e-11)
        _within("s update_scaling rti' r = I", T.T @ R, np.eye(m), 1e-11)
        _within("s update_scaling U' U = I", U[i].T @ U[i], np.eye(m), 1e-11)
        _within("s update_scaling V' V = I", Vt[i] @ Vt[i].T, np.eye(m), 1e-11)
        _within("s update_scaling U diag(l) V' = Lz' Ls", U[i] @ np.diag(lmk) @ Vt[i], M, 1e-11)      # (a wrong vt store fails here)
        il += m


@pytest.mark.parametrize("mnl", MNL_S)
def test_s_scale_all_forms_on_three_padded_columns(mnl):
    C = s_case(mnl)
    W = _s_scaling(mnl)
    Rl, Tl = [_ld(r.a) for r in W["r"]], [_ld(r.a) for r in W["rti"]]
    for tr in "NT":
        for inv in "NI":
            def run():
                x = matrix(C.X.copy(order="F"))
                misc.scale(x, W, trans=tr, inverse=inv)
                return [x.a.copy()]
            got = _twice(run)[0]
            assert got[C.N:].tobytes() == C.X[C.N:].tobytes()
            for c in range(3):
                Gb, Xb = _sblocks(got[:, c], C.nlq), _sblocks(C.X[:, c], C.nlq)
                for i, m in enumerate(SD):
                    ref = orc.scale_s(_ld(Xb[i]), Rl[i], Tl[i], tr, inv)
                    _within("s scale %s%s" % (tr, inv), np.tril(Gb[i]), np.tril(ref), 1e-12)
                    assert np.triu(Gb[i], 1).tobytes() == np.triu(Xb[i], 1).tobytes(), (tr, inv, c, m)


@pytest.mark.parametrize("mnl", MNL_S)
def test_s_scale2_sprod_sinv_ssqr(mnl):
    C = s_case(mnl)
    nlq, x1, y1 = C.nlq, C.x1, C.y1
    Xb, Yb = _sblocks(x1, nlq), _sblocks(y1, nlq)
    off1 = np.concatenate([[0], np.cumsum(SD)]) + nlq
    for inv in "NI":
        got = _twice(lambda: [_run_on(x1, lambda a: misc.scale2(matrix(C.lmd), a, C.dims, C.k, inverse=inv))])[0]
        for i, B in enumerate(_sblocks(got, nlq)):
            _within("s scale2 " + inv, B, orc.scale2_s(_ld(C.lmd[off1[i]:off1[i + 1]]), _ld(Xb[i]), inv), 1e-12)

    def run():
        a, b = matrix(x1.copy()), matrix(y1.copy())
        misc.sprod(a, b, C.dims, C.k)
        return [a._a.copy(), b._a.copy()]
    got, yafter = _twice(run)
    for i, B in enumerate(_sblocks(got, nlq)):
        ref = orc.sprod_s(_ld(Xb[i]), _ld(Yb[i]))
        _within("s sprod", np.tril(B), np.tril(ref), 1e-12)
        assert np.triu(B, 1).tobytes() == np.triu(Xb[i], 1).tobytes()
        Ya = _sblocks(yafter, nlq)[i]                        # y leaves with its upper triangle the mirror of its lower one
        assert Ya.tobytes() == (np.tril(Yb[i]) + np.tril(Yb[i], -1).T).tobytes()
    for name, fn, oracle in (("s sprod D", lambda a: misc.sprod(a, matrix(C.yd), C.dims, C.k, diag="D"), lambda X, y: orc.sprod_s(X, y, "D")),
                             ("s sinv", lambda a: misc.sinv(a, matrix(C.yd), C.dims, C.k), orc.sinv_s)):
        got = _twice(lambda: [_run_on(x1, fn)])[0]
        for i, B in enumerate(_sblocks(got, nlq)):
            ref = oracle(_ld(Xb[i]), _ld(C.yd[off1[i]:off1[i + 1]]))
            _within(name, np.tril(B), np.tril(ref), 1e-12)
            assert np.triu(B, 1).tobytes() == np.triu(Xb[i], 1).tobytes()
    got = _twice(lambda: [_run_on(np.zeros(C.Nd), lambda a: misc.ssqr(a, matrix(C.yd), C.dims, C.k))])[0]
    _within("s ssqr", got[nlq:], orc.ssqr_l(_ld(C.yd[nlq:])), 1e-12)


def _run_on(x, fn):
    a = matrix(x.copy())
    fn(a)
    return a._a.copy()


@pytest.mark.parametrize("mnl", MNL_S)
def test_s_sdot_block_by_block(mnl):
    C = s_case(mnl)
    nlq, x1, y1 = C.nlq, C.x1, C.y1
    Xb, Yb = [_ld(B) for B in _sblocks(x1, nlq)], [_ld(B) for B in _sblocks(y1, nlq)]
    ref = [orc.sdot_s(X, Y) for X, Y in zip(Xb, Yb)]
    sabs = [float(orc.sdot_s(np.abs(X), np.abs(Y))) for X, Y in zip(Xb, Yb)]
    got = _twice(lambda: [np.array(misc.sdot(matrix(x1), matrix(y1), C.dims, C.k))])[0]
    _within("s sdot", got, np.dot(_ld(x1[:nlq]), _ld(y1[:nlq])) + sum(ref), 1e-12, scale=float(np.sum(np.abs(x1[:nlq] * y1[:nlq]))) + sum(sabs))
    o = nlq
    for i, m in enumerate(SD):                                # one block at a time: zeros everywhere else
        xm = np.zeros(C.N)
        xm[o:o + m * m] = x1[o:o + m * m]
        _within("s sdot", misc.sdot(matrix(xm), matrix(y1), C.dims, C.k), ref[i], 1e-12, scale=sabs[i])
        o += m * m


@pytest.mark.parametrize("mnl", MNL_S)
def test_s_storage_helpers_bit_for_bit(mnl):
    C = s_case(mnl)
    nlq, k, x1, y1 = C.nlq, C.k, C.x1, C.y1
    Xb, Yb = _sblocks(x1, nlq), _sblocks(y1, nlq)

    def run():
        yp = matrix(5.0, (C.Np + 5, 1))
        misc.pack(matrix(np.concatenate([[9.0], x1])), yp, C.dims, k, 1, 2)
        yu = matrix(7.0, (C.N + 4, 1))
        misc.unpack(yp, yu, C.dims, k, 2, 3)
        x2 = matrix(np.column_stack([x1, y1]).copy(order="F"))
        misc.pack2(x2, C.dims, k)
        a, b = matrix(x1.copy()), matrix(x1.copy())
        misc.trisc(a, C.dims, k)
        misc.triusc(b, C.dims, k)
        c, o = matrix(x1.copy()), nlq
        for m in SD:
            misc.symm(c, m, o)
            o += m * m
        return [yp._a.copy(), yu._a.copy(), x2.a.copy(), a._a.copy(), b._a.copy(), c._a.copy()]
    yp, yu, x2, tri, triu, sym = _twice(run)
    packed = np.concatenate([orc.pack_s(B) for B in Xb])
    assert yp.tobytes() == np.concatenate([[5.0, 5.0], x1[:nlq], packed, [5.0, 5.0, 5.0]]).tobytes()
    ip, unp = 0, []
    for m in SD:
        unp.append(orc.unpack_s(packed[ip:ip + m * (m + 1) // 2], np.full((m, m), 7.0)).reshape(-1, order="F"))
        ip += m * (m + 1) // 2
    assert yu.tobytes() == np.concatenate([[7.0] * 3, x1[:nlq]] + unp + [[7.0]]).tobytes()
    for c, (v, blocks) in enumerate(((x1, Xb), (y1, Yb))):
        want = np.concatenate([v[:nlq]] + [orc.pack2_s(B) for B in blocks] + [v[C.Np:]])
        assert x2[:, c].tobytes() == want.tobytes()
    for got, fn in ((tri, orc.trisc_s), (triu, orc.triusc_s), (sym, orc.symm_s)):
        want = np.concatenate([x1[:nlq]] + [fn(B).reshape(-1, order="F") for B in Xb])
        assert np.array_equal(got, want) and got[:nlq].tobytes() == x1[:nlq].tobytes()


# ---- end to end through the resident-vector driver (cone.py calls the same kernels without misc) -------------------------------
def test_conelp_one_second_order_cone_of_order_300():
    """minimize c'x subject to |x|_2 <= 1 (n = 299): x = -c / |c|."""
    n = 299
    c = np.random.default_rng(41).standard_normal(n)
    G = np.zeros((n + 1, n))
    G[1:, :] = -np.eye(n)
    h = np.zeros(n + 1)
    h[0] = 1.0
    sol = solvers.conelp(matrix(c), matrix(np.asfortranarray(G)), matrix(h), {"l": 0, "q": [n + 1], "s": []},
                         options={"show_progress": False})
    assert sol["status"] == "optimal"
    x, want = np.asarray(sol["x"]).reshape(-1), -c / np.linalg.norm(c)
    _within("conelp 'q' order 300 x", x, want, 1e-6, scale=max(1.0, float(np.abs(want).max())))
    _scalar("conelp 'q' order 300 objective", np.dot(c, x), -np.linalg.norm(c), 1e-6)


def test_conelp_one_semidefinite_block_of_order_65():
    """minimize t subject to t I - A >= 0 (A symmetric of order 65): t = the largest eigenvalue of A."""
    m = 65
    B = np.random.default_rng(42).standard_normal((m, m))
    A = 0.5 * (B + B.T)
    G = -np.eye(m).reshape(-1, 1, order="F")
    h = -A.reshape(-1, order="F")
    sol = solvers.conelp(matrix(np.array([1.0])), matrix(np.asfortranarray(G)), matrix(h), {"l": 0, "q": [], "s": [m]},
                         options={"show_progress": False})
    assert sol["status"] == "optimal"
    _scalar("conelp 's' order 65 t", np.asarray(sol["x"]).reshape(-1)[0], np.linalg.eigvalsh(A)[-1], 1e-6)
