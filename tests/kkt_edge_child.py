"""The device side of tests/test_kkt_edges_gpu.py: the cases of kkt_edge_cases.py through the `_dev` entries of the C ABI (ctypes),
and, run as a program, the child process of that file -- the library reads KVX_LP_UNFUSED and KVX_ATDA_LPE once per process, so
every setting is a process of its own (the parent sets it):

    python kkt_edge_child.py digest     sections 2 and 5 on the cases' seeds; prints one JSON line {case: sha1 of the outputs' bytes}
    python kkt_edge_child.py atda       the assembly cases against the bound; prints one JSON line {"ratio": largest error / bound}

Every device buffer is PAD doubles longer than its data; the tail holds a sentinel that must survive (Buf.get, Buf.check, and
Buf.check_all at the end of every test and of every case of the child), and the rows between n and the leading dimension of a
strided output hold it too.  Outputs start as NaN, so an entry that is not written
fails the comparison."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import kkt_edge_cases as kc                 # noqa: E402
from kkt_edge_cases import LD               # noqa: E402
from kvxopt_amd import _lib                 # noqa: E402

SENT_BITS = np.array([kc.SENTINEL]).view(np.int64)[0]


def ok(rc):
    _lib.raise_for(rc)


class Buf:
    """an HBM buffer of 8-byte items with the sentinel tail; every buffer stays in `live` until check_all has seen its tail"""
    live = []

    def __init__(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.dtype.itemsize == 8
        self.n, self.dtype = a.size, a.dtype
        self.dev = _lib.DeviceBuffer(8 * (self.n + kc.PAD))
        self.dev.upload(np.concatenate([a.view(np.int64), np.full(kc.PAD, SENT_BITS, dtype=np.int64)]))
        Buf.live.append(self)

    @classmethod
    def nan(cls, n):
        return cls(np.full(int(n), np.nan))

    @property
    def ptr(self):
        return self.dev.ptr

    def get(self):
        raw = self.dev.download(np.int64, self.n + kc.PAD)
        assert np.all(raw[self.n:] == SENT_BITS), "the sentinel behind a buffer of %d items was overwritten" % self.n
        return raw[:self.n].view(self.dtype).copy()

    def check(self):
        """the tail alone"""
        tail = np.empty(kc.PAD, dtype=np.int64)
        ok(_lib.lib().kvx_dev_download(tail.ctypes.data, self.dev.ptr + 8 * self.n, tail.nbytes))
        assert np.all(tail == SENT_BITS), "the sentinel behind a buffer of %d items was overwritten" % self.n

    @classmethod
    def check_all(cls):
        """the tail of every buffer made since the last call (the end of a test, of a case in the child)"""
        bufs, cls.live = cls.live, []
        for b in bufs:
            b.check()


def strided(cols, ld):
    """(Buf, read) of the columns stacked with leading dimension ld, the padding rows holding the sentinel; read() returns the columns
    after checking the padding"""
    n, k = len(cols[0]), len(cols)
    X = np.full((ld, k), kc.SENTINEL, order="F")
    for c in range(k):
        X[:n, c] = cols[c]
    b = Buf(X.reshape(-1, order="F"))

    def read():
        Y = b.get().reshape((ld, k), order="F")
        assert np.all(Y[n:, :].view(np.int64) == SENT_BITS), "a padding row of a strided buffer was overwritten"
        return [Y[:n, c].copy() for c in range(k)]
    return b, read


def ccs_dev(mat):
    return Buf(mat.cp), Buf(mat.ri if len(mat.ri) else np.zeros(1, dtype=np.int64)), Buf(mat.vx if len(mat.vx) else np.zeros(1))


class Ratios(dict):
    def put(self, name, got, out):
        self[name] = kc.ratio(got, out)
        assert self[name] <= 1.0, "%s: error / bound = %.3g" % (name, self[name])

    def put_all(self, prefix, bufs, outs):
        assert set(bufs) == set(outs), (sorted(bufs), sorted(outs))
        for k in outs:
            self.put(prefix + "." + k, bufs[k].get() if isinstance(bufs[k], Buf) else bufs[k], outs[k])

    def worst(self):
        return max(self.values(), default=0.0)


# ---- 1. elementwise ----------------------------------------------------------------------------------------------------------
def run_elementwise(n):
    L = _lib.lib()
    v = kc.elem_data(n)
    R = Ratios()
    B = lambda key: Buf(v[key])
    # NT scaling
    s, z, d, di, lm = B("s"), B("z"), Buf.nan(n), Buf.nan(n), Buf.nan(n)
    ok(L.kvx_nt_compute_scaling_dev(n, s.ptr, z.ptr, d.ptr, di.ptr, lm.ptr))
    R.put_all("compute_scaling", dict(d=d, di=di, lm=lm), kc.e_compute_scaling(LD, v["s"], v["z"]))
    s.check(); z.check()
    s, z, d, di, lm = B("s"), B("z"), B("d"), Buf.nan(n), Buf.nan(n)
    ok(L.kvx_nt_update_scaling_dev(n, s.ptr, z.ptr, d.ptr, di.ptr, lm.ptr))
    R.put_all("update_scaling", dict(s=s, z=z, d=d, di=di, lm=lm), kc.e_update_scaling(LD, v["s"], v["z"], v["d"]))
    # Newton right-hand side, four forms
    rz, lmb, db, lsq, ws3 = B("rz"), B("lm"), B("d"), B("lsq"), B("ws3")
    for with_lsq in (True, False):
        for with_ws3 in (True, False):
            ds, dz = Buf.nan(n), Buf.nan(n)
            ok(L.kvx_lp_newton_rhs_dev(n, lsq.ptr if with_lsq else None, ws3.ptr if with_ws3 else None, v["shift"], v["scale"], rz.ptr,
                                       lmb.ptr, db.ptr, ds.ptr, dz.ptr))
            R.put_all("newton_rhs[lsq=%d,ws3=%d]" % (with_lsq, with_ws3), dict(ds=ds, dz=dz),
                      kc.e_newton_rhs(LD, v["lsq"] if with_lsq else None, v["ws3"] if with_ws3 else None, v["shift"], v["scale"], v["rz"],
                                      v["lm"], v["d"]))
    for b in (rz, lmb, db, lsq, ws3):
        b.check()
    # step_post with and without ws3
    z1 = B("z1")
    for with_ws3 in (True, False):
        ds, dz, w3 = B("ds"), B("dz"), Buf.nan(n)
        ok(L.kvx_lp_step_post_dev(n, v["dtau"], z1.ptr, lmb.ptr, ds.ptr, dz.ptr, w3.ptr if with_ws3 else None))
        bufs = dict(ds=ds, dz=dz, ws3=w3) if with_ws3 else dict(ds=ds, dz=dz)
        R.put_all("step_post[ws3=%d]" % with_ws3, bufs, kc.e_step_post(LD, v["dtau"], v["z1"], v["lm"], v["ds"], v["dz"], with_ws3))
        if not with_ws3:
            assert np.all(np.isnan(w3.get()))
    # the update at the end of an iteration
    ds, dz, d, di, lm, s, z = B("dsp"), B("dzp"), B("d"), Buf.nan(n), B("lm"), Buf.nan(n), Buf.nan(n)
    ok(L.kvx_lp_update_dev(n, v["step"], ds.ptr, dz.ptr, d.ptr, di.ptr, lm.ptr, s.ptr, z.ptr))
    R.put_all("lp_update", dict(ds=ds, dz=dz, d=d, di=di, lm=lm, s=s, z=z), kc.e_lp_update(LD, v["step"], v["dsp"], v["dzp"], v["d"], v["lm"]))
    # scale: 1 and 3 columns, ldx > n
    cols = [v["x"], v["y"], v["zz"]]
    for ncols in (1, 3):
        xb, read = strided(cols[:ncols], n + 3)
        ok(L.kvx_nt_scale_dev(n, ncols, n + 3, xb.ptr, lmb.ptr))
        for c, got in enumerate(read()):
            R.put("scale[%d cols].%d" % (ncols, c), got, kc.e_mul(LD, cols[c], v["lm"]))
    for inverse, f in ((0, kc.e_div), (1, kc.e_mul)):
        x = B("x")
        ok(L.kvx_nt_scale2_dev(n, lmb.ptr, x.ptr, inverse))
        R.put("scale2[inverse=%d]" % inverse, x.get(), f(LD, v["x"], v["lm"]))
    x, y = B("x"), B("y")
    ok(L.kvx_nt_sprod_dev(n, x.ptr, y.ptr))
    R.put("sprod", x.get(), kc.e_mul(LD, v["x"], v["y"]))
    x = B("x")
    ok(L.kvx_nt_sinv_dev(n, x.ptr, lmb.ptr))
    R.put("sinv", x.get(), kc.e_div(LD, v["x"], v["lm"]))
    x = Buf.nan(n)
    ok(L.kvx_nt_ssqr_dev(n, x.ptr, y.ptr))
    R.put("ssqr", x.get(), kc.e_mul(LD, v["y"], v["y"]))
    # BLAS-1 glue
    x, y = B("x"), B("y")
    ok(L.kvx_vec_axpy_dev(n, v["a"], x.ptr, y.ptr))
    R.put("axpy", y.get(), kc.e_axpy(LD, v["a"], v["x"], v["y"]))
    y, zb = B("y"), Buf.nan(n)
    ok(L.kvx_vec_lincomb_dev(n, v["a"], x.ptr, v["b"], y.ptr, zb.ptr))
    R.put("lincomb", zb.get(), kc.e_lincomb(LD, v["a"], v["x"], v["b"], v["y"]))
    ynan, zb = Buf.nan(n), Buf.nan(n)
    ok(L.kvx_vec_lincomb_dev(n, v["a"], x.ptr, 0.0, ynan.ptr, zb.ptr))                        # b = 0: y is not read
    R.put("lincomb[b=0]", zb.get(), kc.e_lincomb(LD, v["a"], v["x"], 0.0, None))
    xa = B("x")
    ok(L.kvx_vec_lincomb_dev(n, v["a"], xa.ptr, v["b"], y.ptr, xa.ptr))                       # z is x
    R.put("lincomb[z=x]", xa.get(), kc.e_lincomb(LD, v["a"], v["x"], v["b"], v["y"]))
    ya = B("y")
    ok(L.kvx_vec_lincomb_dev(n, v["a"], x.ptr, v["b"], ya.ptr, ya.ptr))                       # z is y
    R.put("lincomb[z=y]", ya.get(), kc.e_lincomb(LD, v["a"], v["x"], v["b"], v["y"]))
    xa = B("x")
    ok(L.kvx_vec_scal_dev(n, v["a"], xa.ptr))
    R.put("scal", xa.get(), kc.e_scal(LD, v["a"], v["x"]))
    xa = B("x")
    ok(L.kvx_vec_addc_dev(n, v["c"], xa.ptr))
    R.put("addc", xa.get(), kc.e_addc(LD, v["c"], v["x"]))
    xa = Buf.nan(n)
    ok(L.kvx_vec_fill_dev(n, v["c"], xa.ptr))
    assert kc.same_bits(xa.get(), np.full(n, v["c"])), "fill"
    zb = B("zz")
    ok(L.kvx_vec_xmy_dev(n, v["a"], x.ptr, y.ptr, v["b"], zb.ptr))
    R.put("xmy", zb.get(), kc.e_xmy(LD, v["a"], v["x"], v["y"], v["b"], v["zz"]))
    zb = Buf.nan(n)
    ok(L.kvx_vec_xmy_dev(n, v["a"], x.ptr, y.ptr, 0.0, zb.ptr))                               # b = 0: z is not read
    R.put("xmy[b=0]", zb.get(), kc.e_xmy(LD, v["a"], v["x"], v["y"], 0.0, None))
    src = np.random.default_rng(n).standard_normal(3 * n - 2)
    sb, out = Buf(src), Buf.nan(n)
    ok(L.kvx_vec_copy_strided_dev(n, sb.ptr, 3, out.ptr))
    assert kc.same_bits(out.get(), src[::3]), "copy_strided"
    x.check(); y.check(); sb.check()
    return R


# ---- 2. reductions -------------------------------------------------------------------------------------------------------------
def sdot(n, x, y):
    r = ctypes.c_double()
    ok(_lib.lib().kvx_nt_sdot_dev(n, x.ptr, y.ptr, ctypes.byref(r)))
    return r.value


def max_step(n, x):
    r = ctypes.c_double()
    ok(_lib.lib().kvx_nt_max_step_dev(n, x.ptr, ctypes.byref(r)))
    return r.value


def reduce_multi(slots):
    """slots: [(kind, n, xbuf, ybuf)] -> (return code, values)"""
    m = len(slots)
    kind = (ctypes.c_int32 * max(m, 1))(*[s[0] for s in slots])
    nn = (ctypes.c_int64 * max(m, 1))(*[s[1] for s in slots])
    xs = (ctypes.c_void_p * max(m, 1))(*[s[2].ptr for s in slots])
    ys = (ctypes.c_void_p * max(m, 1))(*[(s[3].ptr if s[0] == 0 else None) for s in slots])
    res = (ctypes.c_double * max(m, 1))()
    rc = _lib.lib().kvx_nt_reduce_multi_dev(m, kind, nn, xs, ys, res)
    return rc, [float(res[i]) for i in range(m)]


def run_reductions(n, check=True):
    """-> (ratios, values): sdot, max_step with the extreme element planted at every edge, max_step of a positive vector"""
    x, y = kc.red_data(n)
    R, vals = Ratios(), {}
    xb, yb = Buf(x), Buf(y)
    vals["dot"] = sdot(n, xb, yb)
    if check:
        R.put("dot[%d]" % n, [vals["dot"]], kc.r_dot(LD, x, y))
    vals["max"] = max_step(n, xb)
    if check:
        assert kc.same_bits([vals["max"]], [kc.r_max_step(x)]), ("max_step", n)
    for name, idx in sorted(kc.max_step_plants(n).items()):
        xp = x.copy()
        xp[idx] = -5.0e3                                          # every other magnitude is at most 1e3
        pb = Buf(xp)
        vals["max@" + name] = max_step(n, pb)
        if check:
            assert vals["max@" + name] == 5.0e3, ("max_step misses the element at %d (%s) of %d" % (idx, name, n), vals["max@" + name])
        pb.check()
    xpos = np.abs(x)
    pb = Buf(xpos)
    vals["max_positive"] = max_step(n, pb)
    if check:
        assert vals["max_positive"] == -xpos.min() < 0, ("max_step of a positive vector", n)
    xb.check(); yb.check()
    return R, vals


def run_multi(check=True):
    R, vals = Ratios(), {}
    for name, slots in kc.multi_cases():
        data, args = [], []
        for k, (kind, n) in enumerate(slots):
            x, y = kc.red_data(max(n, 1), seed=101 + k)
            xb, yb = Buf(x), Buf(y)
            data.append((x[:n], y[:n]))
            args.append((kind, n, xb, yb))
        rc, got = reduce_multi(args)
        assert rc == _lib.KVX_OK, (name, rc)
        vals[name] = got
        if not check:
            continue
        for k, (kind, n, xb, yb) in enumerate(args):
            if n == 0:
                assert kind == 0 and kc.same_bits([got[k]], [0.0]), (name, k, got[k])
                continue
            single = sdot(n, xb, yb) if kind == 0 else max_step(n, xb)
            assert kc.same_bits([got[k]], [single]), (name, k, got[k], single)
            if kind == 0:
                R.put("%s.%d" % (name, k), [got[k]], kc.r_dot(LD, *data[k]))
            else:
                assert kc.same_bits([got[k]], [kc.r_max_step(data[k][0])]), (name, k)
            xb.check(); yb.check()
    if check:
        x, y = kc.red_data(5)
        xb, yb = Buf(x), Buf(y)
        rc, _ = reduce_multi([(0, 5, xb, yb)] * 33)
        assert rc == _lib.KVX_EINVAL, rc
        rc, _ = reduce_multi([])
        assert rc == _lib.KVX_OK, rc
    return R, vals


# ---- 3. CCS products --------------------------------------------------------------------------------------------------------
def spmv(trans, mat, dev, alpha, xb, beta, yb):
    ok(_lib.lib().kvx_spmv_dev(ord(trans), mat.m, mat.n, dev[0].ptr, dev[1].ptr, dev[2].ptr, alpha, xb.ptr, beta, yb.ptr))


def run_spmv_t(mat):
    rng = np.random.default_rng(61 + mat.n)
    x, y = kc.spread(rng, mat.m), kc.spread(rng, mat.n)
    dev, xb = ccs_dev(mat), Buf(x)
    R = Ratios()
    for alpha, beta in kc.SPMV_AB:
        yb = Buf.nan(mat.n) if beta == 0 else Buf(y)
        spmv("T", mat, dev, alpha, xb, beta, yb)
        R.put("spmv_t[%s](%g,%g)" % (mat.name, alpha, beta), yb.get(), kc.c_spmv_t(LD, mat, alpha, x, beta, y))
    for b in dev + (xb,):
        b.check()
    return R


def run_spmv_n(mat):
    rng = np.random.default_rng(67 + mat.n)
    x, y = kc.spread(rng, mat.n), kc.spread(rng, mat.m)
    dev, xb = ccs_dev(mat), Buf(x)
    R = Ratios()
    for beta in (0.0, 1.0, -0.5):
        yb = Buf.nan(mat.m) if beta == 0 else Buf(y)
        spmv("N", mat, dev, 2.0, xb, beta, yb)
        R.put("spmv_n[%s](2,%g)" % (mat.name, beta), yb.get(), kc.c_spmv_n(LD, mat, 2.0, x, beta, y))
    for b in dev + (xb,):
        b.check()
    return R


def run_spmm_t(mat):
    """1 and 3 columns with ldx, ldy larger than needed: every column to the bound and bit for bit kvx_spmv_dev 'T' with (1, 0)"""
    rng = np.random.default_rng(71)
    cols = [kc.spread(rng, mat.m) for _ in range(3)]
    dev = ccs_dev(mat)
    R = Ratios()
    solo = []
    for c in range(3):
        xb, yb = Buf(cols[c]), Buf.nan(mat.n)
        spmv("T", mat, dev, 1.0, xb, 0.0, yb)
        solo.append(yb.get())
    for ncols in (1, 3):
        ldx, ldy = mat.m + 5, mat.n + 7
        xb, _ = strided(cols[:ncols], ldx)
        yb, read = strided([np.full(mat.n, np.nan)] * ncols, ldy)
        ok(_lib.lib().kvx_spmm_t_dev(mat.n, ncols, dev[0].ptr, dev[1].ptr, dev[2].ptr, xb.ptr, ldx, yb.ptr, ldy))
        for c, got in enumerate(read()):
            R.put("spmm_t[%d cols].%d" % (ncols, c), got, kc.c_spmv_t(LD, mat, 1.0, cols[c], 0.0, None))
            assert kc.same_bits(got, solo[c]), ("spmm_t column %d of %d differs from spmv 'T'" % (c, ncols))
        xb.check()
    return R


def run_dense_gemv(m):
    rng = np.random.default_rng(73 + m)
    R = Ratios()
    for n in kc.GEMV_N:
        lda, ldx, ldy = m + 3, n + 2, m + 5
        A = kc.spread(rng, m * max(n, 1)).reshape(m, max(n, 1))[:, :n]
        Ab, _ = strided([A[:, j] for j in range(n)], lda) if n else (Buf(np.zeros(1)), None)
        for nrhs in (1, 3):
            xs = [kc.spread(rng, n) for _ in range(nrhs)]
            ys = [kc.spread(rng, m) for _ in range(nrhs)]
            xb, _ = strided(xs, ldx)
            for beta in (0.0, -0.5):
                yb, read = strided([np.full(m, np.nan)] * nrhs if beta == 0 else ys, ldy)
                ok(_lib.lib().kvx_dense_gemv_dev(m, n, nrhs, 1.5, Ab.ptr, lda, xb.ptr, ldx, beta, yb.ptr, ldy))
                for c, got in enumerate(read()):
                    R.put("gemv[m=%d,n=%d,nrhs=%d,beta=%g].%d" % (m, n, nrhs, beta, c), got, kc.c_dense_gemv(LD, A, xs[c], 1.5, beta, ys[c]))
            xb.check()
        Ab.check()
    return R


def run_dense_and_pack(p):
    """kvx_dense_from_ccs_dev of a p x p CCS matrix (an empty column among them) and kvx_pack_lower_dev of the dense result, ld > p:
    exact"""
    rng = np.random.default_rng(79 + p)
    lens = np.minimum(kc.lens_cycle(p, [1, 2, 0, 5, 3], empty_ends=False), p)
    if p > 2:
        lens[-1] = p                                              # a full column
    cp, ri, vx = _any_rows(rng, p, lens)
    mat = kc.Mat("d%d" % p, p, p, cp, ri, vx)
    dev = ccs_dev(mat)
    ld = p + 3
    Db, read = strided([np.full(p, np.nan)] * p, ld)
    ok(_lib.lib().kvx_dense_from_ccs_dev(p, p, dev[0].ptr, dev[1].ptr, dev[2].ptr, Db.ptr, ld))
    D = np.stack(read(), axis=1)
    ref = kc.dense_of(p, p, cp, ri, vx, np.float64)
    assert kc.same_bits(np.ascontiguousarray(D), np.ascontiguousarray(ref)), ("dense_from_ccs", p)
    # pack the lower triangle of a matrix without zeros
    K = kc.spread(rng, p * p).reshape(p, p)
    Kb, _ = strided([K[:, j] for j in range(p)], ld)
    out = Buf.nan(p * (p + 1) // 2)
    ok(_lib.lib().kvx_pack_lower_dev(p, Kb.ptr, ld, out.ptr))
    assert kc.same_bits(out.get(), np.concatenate([K[j:, j] for j in range(p)])), ("pack_lower", p)
    Kb.check()
    for b in dev:
        b.check()


def _any_rows(rng, m, lens):
    """as kc.ccs_by_lengths for an m that is not prime: consecutive rows from a random start (mod m)"""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    cp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.repeat(np.arange(n, dtype=np.int64), lens)
    k = np.arange(cp[-1], dtype=np.int64) - cp[col]
    ri = (rng.integers(0, m, n)[col] + k) % m
    order = np.lexsort((ri, col))
    return cp, np.ascontiguousarray(ri[order]), kc.spread(rng, cp[-1])


# ---- 4. assembly ---------------------------------------------------------------------------------------------------------------
def plan(case, Pp=None, Pi=None):
    L = _lib.lib()
    Pp = case.Pp if Pp is None else Pp
    Pi = case.Pi if Pi is None else Pi
    h = ctypes.c_void_p()
    Gi = case.Gi if len(case.Gi) else np.zeros(1, dtype=np.int64)
    ok(L.kvx_atda_plan(case.ml, case.n, _lib.pi(case.Gp), _lib.pi(Gi), _lib.pi(Pp) if Pp is not None else None,
                       _lib.pi(Pi if len(Pi) else np.zeros(1, dtype=np.int64)) if Pp is not None else None, ctypes.byref(h)))
    snz = ctypes.c_int64()
    ok(L.kvx_atda_pattern(h, ctypes.byref(snz), None, None))
    Sp, Si = np.empty(case.n + 1, dtype=np.int64), np.empty(max(snz.value, 1), dtype=np.int64)
    ok(L.kvx_atda_pattern(h, ctypes.byref(snz), _lib.pi(Sp), _lib.pi(Si)))
    return h, Sp, Si[:snz.value]


def assemble_dev(h, snz, gx, w, px, sq=False):
    f = _lib.lib().kvx_atda_assemble_sq_dev if sq else _lib.lib().kvx_atda_assemble_dev
    sx = Buf.nan(snz)
    ok(f(h, gx.ptr, w.ptr, px.ptr if px is not None else None, sx.ptr))
    return sx.get()


def run_assembly(case, bits=True):
    """one case to the bound -> (ratios, the values of S); bits: the equalities of the default schedule as well"""
    L = _lib.lib()
    R = Ratios()
    h, Sp, Si = plan(case)
    try:
        eSp, eSi, lens = kc.atda_pattern(case)
        assert np.array_equal(Sp, eSp) and np.array_equal(Si, eSi), ("pattern", case.name)
        snz = len(Si)
        gx, w = Buf(case.Gx if len(case.Gx) else np.zeros(1)), Buf(case.w)
        px = Buf(case.Px) if case.Px is not None else None
        ref, _ = kc.a_assemble(LD, case)
        got = assemble_dev(h, snz, gx, w, px)
        R.put("assemble[%s]" % case.name, got, ref)
        ref0 = ref.ref.astype(np.float64)
        assert kc.same_bits(got[lens == 0], ref0[lens == 0]), ("an entry that only P brings", case.name)
        refq, _ = kc.a_assemble(LD, case, sq=True)
        gotq = assemble_dev(h, snz, gx, w, px, sq=True)
        R.put("assemble_sq[%s]" % case.name, gotq, refq)
        if bits:
            assert kc.same_bits(assemble_dev(h, snz, gx, w, px), got), ("two assemblies", case.name)
            w2 = Buf.nan(case.ml)
            ok(L.kvx_nt_ssqr_dev(case.ml, w2.ptr, w.ptr))
            assert kc.same_bits(assemble_dev(h, snz, gx, w2, px), gotq), ("assemble_sq_dev against ssqr + assemble_dev", case.name)
            host = np.full(max(snz, 1), np.nan)
            ok(L.kvx_atda_assemble(h, _lib.pd(case.Gx if len(case.Gx) else np.zeros(1)), _lib.pd(case.w),
                                   _lib.pd(case.Px) if case.Px is not None else None, _lib.pd(host)))
            assert kc.same_bits(host[:snz], got), ("the host entry against the device entry", case.name)
        for b in (gx, w) + ((px,) if px is not None else ()):
            b.check()
    finally:
        L.kvx_atda_free(h)
    return R, got


def run_assembly_p_contract(case):
    """The contract of the header for P on a case with a lower-triangular P: the lower triangle is read.  (a) P given as a full
    symmetric matrix gives the bits of its lower triangle; (b) an entry above the diagonal -- (0, n - 1), which the plan before
    the fix sent to slot 0, the head of column 0 -- changes nothing; (c) a position stored twice: the sum in the order stored, to the
    bound, and two runs with the same bits."""
    L = _lib.lib()
    R = Ratios()
    n = case.n
    gx, w = Buf(case.Gx), Buf(case.w)
    h, Sp, Si = plan(case)
    base = assemble_dev(h, len(Si), gx, w, Buf(case.Px))
    L.kvx_atda_free(h)
    pc = np.repeat(np.arange(n), np.diff(case.Pp))

    def variant(rows, cols, vals):
        """CCS in the order given within a column"""
        order = np.argsort(cols, kind="stable")
        rows, cols, vals = rows[order], cols[order], vals[order]
        Pp = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(cols, minlength=n), out=Pp[1:])
        return Pp, np.ascontiguousarray(rows), np.ascontiguousarray(vals)

    strict = case.Pi > pc
    # (a) the full symmetric matrix: the mirrored entries first within their columns
    Pp, Pi, Px = variant(np.concatenate([pc[strict], case.Pi]), np.concatenate([case.Pi[strict], pc]),
                         np.concatenate([case.Px[strict], case.Px]))
    h, Sp2, Si2 = plan(case, Pp, Pi)
    assert np.array_equal(Sp2, Sp) and np.array_equal(Si2, Si), "the pattern with a full P"
    full = assemble_dev(h, len(Si), gx, w, Buf(Px))
    L.kvx_atda_free(h)
    assert kc.same_bits(full, base), "P as a full symmetric matrix against its lower triangle"
    # (b) one entry above the diagonal, in the first row
    Pp, Pi, Px = variant(np.concatenate([[0], case.Pi]), np.concatenate([[n - 1], pc]), np.concatenate([[977.0], case.Px]))
    h, Sp2, Si2 = plan(case, Pp, Pi)
    assert np.array_equal(Sp2, Sp) and np.array_equal(Si2, Si), "the pattern with an upper entry"
    up = assemble_dev(h, len(Si), gx, w, Buf(Px))
    L.kvx_atda_free(h)
    assert kc.same_bits(up, base), "an entry of P above the diagonal contributes"
    # (c) positions stored twice and three times: the diagonal head (0, 0) and an off-diagonal entry
    k = int(np.flatnonzero(strict)[0])
    rows = np.concatenate([case.Pi, [0, case.Pi[k], 0]])
    cols = np.concatenate([pc, [0, pc[k], 0]])
    vals = np.concatenate([case.Px, [-417.5, 0.00390625 * 3, 88.25]])
    Pp, Pi, Px = variant(rows, cols, vals)
    h, Sp2, Si2 = plan(case, Pp, Pi)
    assert np.array_equal(Sp2, Sp) and np.array_equal(Si2, Si), "the pattern with repeated positions"
    pxb = Buf(Px)
    rep1 = assemble_dev(h, len(Si), gx, w, pxb)
    rep2 = assemble_dev(h, len(Si), gx, w, pxb)
    L.kvx_atda_free(h)
    ref, _ = kc.a_assemble(LD, case, Px=Px, Pp=Pp, Pi=Pi)
    R.put("assemble[%s, repeated P]" % case.name, rep1, ref)
    assert kc.same_bits(rep1, rep2), "two runs with a repeated position"
    assert not kc.same_bits(rep1, base)
    return R


# ---- 5. fused kernels ------------------------------------------------------------------------------------------------------
def sides(items):
    arr = (_lib.KktSide * 2)()
    for k, (xin, xs, zin, xout, xos, zout, zos) in enumerate(items):
        a = arr[k]
        a.xin, a.xscale, a.zin = xin.ptr, float(xs), zin.ptr
        a.xout, a.xoscale, a.zout, a.zoscale = xout.ptr, float(xos), zout.ptr, float(zos)
    return arr


XS, XOS, ZOS = (-0.75, 1.25), (0.625, -2.5), (-1.5, 0.375)


def fused_data(mat):
    rng = np.random.default_rng(83 + mat.m + 3 * mat.n)
    sp = lambda n, **kw: kc.spread(rng, n, **kw)
    return dict(di=sp(mat.m, signed=False), xin=[sp(mat.n), sp(mat.n)], zin=[sp(mat.m), sp(mat.m)], x2=[sp(mat.n), sp(mat.n)],
                x=sp(mat.n), z=sp(mat.m), s=sp(mat.m), c=sp(mat.n), h=sp(mat.m), tau=0.8125)


def fused_calls(mat, v, hint_col, hint_row, nrhs, ldx2):
    """pre, post and residuals with the given lane hints -> the outputs as arrays"""
    L = _lib.lib()
    tmat = kc.transpose_ccs(mat.m, mat.n, mat.cp, mat.ri, mat.vx)
    g = ccs_dev(mat)
    t = ccs_dev(kc.Mat("t", mat.n, mat.m, *tmat))
    di = Buf(v["di"])
    out = {}
    xin, zin = [Buf(a) for a in v["xin"]], [Buf(a) for a in v["zin"]]
    xo, zo = [Buf.nan(mat.n) for _ in range(2)], [Buf.nan(mat.m) for _ in range(2)]
    sd = sides([(xin[k], XS[k], zin[k], xo[k], XOS[k], zo[k], ZOS[k]) for k in range(nrhs)])
    x2, read = strided([np.full(mat.n, np.nan)] * nrhs, ldx2)
    ok(L.kvx_kkt_solve_pre_dev(mat.m, mat.n, g[0].ptr, g[1].ptr, g[2].ptr, hint_col, di.ptr, nrhs, sd, x2.ptr, ldx2))
    out["pre"] = read()
    x2, read = strided(v["x2"][:nrhs], ldx2)
    ok(L.kvx_kkt_solve_post_dev(mat.m, mat.n, t[0].ptr, t[1].ptr, t[2].ptr, hint_row, di.ptr, nrhs, sd, x2.ptr, ldx2))
    read()
    out["xout"] = [xo[k].get() for k in range(nrhs)]
    out["zout"] = [zo[k].get() for k in range(nrhs)]
    ins = [Buf(v[k]) for k in ("x", "z", "s", "c", "h")]
    res = [Buf.nan(mat.n), Buf.nan(mat.n), Buf.nan(mat.m), Buf.nan(mat.m)]
    ok(L.kvx_lp_residuals_dev(mat.m, mat.n, g[0].ptr, g[1].ptr, g[2].ptr, hint_col, t[0].ptr, t[1].ptr, t[2].ptr, hint_row,
                              *[b.ptr for b in ins], v["tau"], *[b.ptr for b in res]))
    for name, b in zip(("hrx", "rx", "hrz", "rz"), res):
        out[name] = b.get()
    for b in g + t + (di,) + tuple(xin) + tuple(zin) + tuple(ins):
        b.check()
    return out, tmat


def check_fused(mat, v, out, tmat, nrhs, R, tag):
    for k in range(nrhs):
        R.put("%s pre.%d" % (tag, k), out["pre"][k], kc.f_pre(LD, mat, v["di"], XS[k], v["xin"][k], v["zin"][k]))
        post = kc.f_post(LD, mat, tmat, v["di"], XOS[k], ZOS[k], v["zin"][k], v["x2"][k])
        R.put("%s post.xout.%d" % (tag, k), out["xout"][k], post["xout"])
        R.put("%s post.zout.%d" % (tag, k), out["zout"][k], post["zout"])
    res = kc.f_residuals(LD, mat, tmat, v["x"], v["z"], v["s"], v["c"], v["h"], v["tau"])
    for name in ("hrx", "rx", "hrz", "rz"):
        R.put("%s %s" % (tag, name), out[name], res[name])


def flat(out):
    return np.concatenate([np.concatenate(a) if isinstance(a, list) else a for _, a in sorted(out.items())])


def run_fused(mat, check=True):
    """pre, post, residuals with the true longest column / row and with 0 (16 lanes): both to the bound, bit-equal where the true
    value is at most the lane count chosen (always, by lanes_for); two right-hand sides with ldx2 > n bit-equal to two single calls"""
    v = fused_data(mat)
    R = Ratios()
    mc, mr = int(np.diff(mat.cp).max()), int(np.bincount(mat.ri, minlength=mat.m).max())
    hinted, tmat = fused_calls(mat, v, mc, mr, 2, mat.n + 3)
    if check:
        check_fused(mat, v, hinted, tmat, 2, R, "%s hinted" % mat.name)
        plain, _ = fused_calls(mat, v, 0, 0, 2, mat.n + 3)
        check_fused(mat, v, plain, tmat, 2, R, "%s 16 lanes" % mat.name)
        for key in sorted(hinted):
            assert kc.same_bits(flat({key: hinted[key]}), flat({key: plain[key]})), ("%d / %d lanes against 16" % (kc.lanes_for(mc), kc.lanes_for(mr)), mat.name, key)
        one, _ = fused_calls(mat, v, mc, mr, 1, mat.n)
        for key in ("pre", "xout", "zout"):
            assert kc.same_bits(one[key][0], hinted[key][0]), ("nrhs = 2 against a single call", mat.name, key)
        # the second side alone: its scalars travel with it
        L = _lib.lib()
        g = ccs_dev(mat)
        t = ccs_dev(kc.Mat("t", mat.n, mat.m, *tmat))
        di, xin, zin, xo, zo = Buf(v["di"]), Buf(v["xin"][1]), Buf(v["zin"][1]), Buf.nan(mat.n), Buf.nan(mat.m)
        sd = sides([(xin, XS[1], zin, xo, XOS[1], zo, ZOS[1])])
        x2 = Buf.nan(mat.n)
        ok(L.kvx_kkt_solve_pre_dev(mat.m, mat.n, g[0].ptr, g[1].ptr, g[2].ptr, mc, di.ptr, 1, sd, x2.ptr, mat.n))
        assert kc.same_bits(x2.get(), hinted["pre"][1]), ("nrhs = 2, second side, pre", mat.name)
        x2 = Buf(v["x2"][1])
        ok(L.kvx_kkt_solve_post_dev(mat.m, mat.n, t[0].ptr, t[1].ptr, t[2].ptr, mr, di.ptr, 1, sd, x2.ptr, mat.n))
        assert kc.same_bits(xo.get(), hinted["xout"][1]) and kc.same_bits(zo.get(), hinted["zout"][1]), ("nrhs = 2, second side, post", mat.name)
    return R, flat(hinted)


def run_fused_big(mat, check=True):
    """past the caps with hint 0, one right-hand side"""
    v = fused_data(mat)
    R = Ratios()
    out, tmat = fused_calls(mat, v, 0, 0, 1, mat.n)
    if check:
        check_fused(mat, v, out, tmat, 1, R, mat.name)
    return R, flat(out)


UPDATE_X_SIZES = [(1, 1), (257, 1), (1, 257), (257, 257), (524289, 257), (257, 524289), (524289, 524289)]


def run_update_x(ml, n, check=True):
    L = _lib.lib()
    rng = np.random.default_rng(89 + ml + 5 * n)
    pos = lambda k: kc.spread(rng, k, signed=False)
    ds, dz, d, lm, x, dx, step = pos(ml), pos(ml), pos(ml), pos(ml), kc.spread(rng, n), kc.spread(rng, n), 0.59375
    bufs = dict(ds=Buf(ds), dz=Buf(dz), d=Buf(d), di=Buf.nan(ml), lm=Buf(lm), s=Buf.nan(ml), z=Buf.nan(ml))
    xb, dxb = Buf(x), Buf(dx)
    ok(L.kvx_lp_update_x_dev(ml, n, step, *[bufs[k].ptr for k in ("ds", "dz", "d", "di", "lm", "s", "z")], dxb.ptr, xb.ptr))
    R = Ratios()
    got = {k: b.get() for k, b in bufs.items()}
    got["x"] = xb.get()
    dxb.check()
    if check:
        R.put_all("update_x[%d,%d]" % (ml, n), {k: got[k] for k in bufs}, kc.e_lp_update(LD, step, ds, dz, d, lm))
        R.put("update_x[%d,%d].x" % (ml, n), got["x"], kc.e_axpy(LD, step, dx, x))
    return R, flat(got)


def run_second_half(ml, n, p, host_zz, with_ws3, check=True):
    """dtau and z1'z1 against the trees' bound, the two step bounds as the exact maxima of the values the device wrote, and dx, dy, ds,
    dz, ws3 as functions of the dtau the device returned, to the elementwise bound"""
    L = _lib.lib()
    v = kc.half_data(ml, n, p)
    zz_in = 2.75 if host_zz else -1.0
    B = {k: Buf(v[k]) for k in ("c", "dx", "x1", "th", "dz", "z1", "ds", "lm", "b", "dy", "y1")}
    ws3 = Buf.nan(ml)
    out = (ctypes.c_double * 4)()
    pp = lambda k: B[k].ptr if p > 0 else None
    ok(L.kvx_lp_second_half_dev(ml, n, p, B["c"].ptr, pp("b"), B["th"].ptr, B["x1"].ptr, pp("y1"), B["z1"].ptr, B["lm"].ptr, B["dx"].ptr, pp("dy"),
                                B["dz"].ptr, B["ds"].ptr, ws3.ptr if with_ws3 else None, v["dgi"], v["dtau0"], zz_in, out))
    dtau, zz, bs, bz = [float(out[i]) for i in range(4)]
    got = dict(dx=B["dx"].get(), dy=B["dy"].get(), ds=B["ds"].get(), dz=B["dz"].get(), ws3=ws3.get())
    for k in ("c", "x1", "th", "z1", "lm", "b", "y1"):
        assert kc.same_bits(B[k].get(), v[k]), ("an input was written", k)
    R = Ratios()
    if check:
        tag = "half[%d,%d,%d]" % (ml, n, p)
        rd, rz = kc.h_dtau(LD, v, ml, n, p, 2.75 if host_zz else None)
        R.put(tag + ".dtau", [dtau], rd)
        if host_zz:
            assert zz == 2.75
        else:
            R.put(tag + ".z1z1", [zz], rz)
        assert kc.same_bits([bs], [np.max(-got["ds"])]) and kc.same_bits([bz], [np.max(-got["dz"])]), (tag, "step bounds")
        post = kc.e_step_post(LD, dtau, v["z1"], v["lm"], v["ds"], v["dz"], with_ws3)
        R.put_all(tag, {k: got[k] for k in post}, post)
        if not with_ws3:
            assert np.all(np.isnan(got["ws3"]))
        R.put(tag + ".dx", got["dx"], kc.e_axpy(LD, dtau, v["x1"], v["dx"]))
        if p > 0:
            R.put(tag + ".dy", got["dy"], kc.e_axpy(LD, dtau, v["y1"][:p], v["dy"][:p]))
        else:
            assert kc.same_bits(got["dy"], v["dy"])
    vals = np.concatenate([[dtau, zz, bs, bz], got["dx"], got["dy"], got["ds"], got["dz"], got["ws3"][~np.isnan(got["ws3"])]])
    return R, vals


# ---- the child ------------------------------------------------------------------------------------------------------------------
def sha(a):
    return hashlib.sha1(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()).hexdigest()


def digest():
    """sections 2 and 5 without the references: the bytes of every output"""
    out = {}

    def put(name, vals):
        out[name] = sha(vals)
        Buf.check_all()

    for n in kc.RED_SIZES:
        _, vals = run_reductions(n, check=False)
        put("red%d" % n, [vals[k] for k in sorted(vals)])
    _, vals = run_multi(check=False)
    for k in sorted(vals):
        put("multi." + k, vals[k])
    for mat in kc.fused_mats():
        put("fused." + mat.name, run_fused(mat, check=False)[1])
    for mat in kc.fused_big_mats():
        put("fused." + mat.name, run_fused_big(mat, check=False)[1])
    for ml, n in UPDATE_X_SIZES:
        put("update_x.%d.%d" % (ml, n), run_update_x(ml, n, check=False)[1])
    for c in kc.half_cases():
        put("half.%d.%d.%d.%d.%d" % c, run_second_half(*c, check=False)[1])
    return out


def atda():
    w = 0.0
    for case in kc.atda_cases():
        R, _ = run_assembly(case, bits=False)
        Buf.check_all()
        w = max(w, R.worst())
    return {"ratio": w, "lpe": os.environ.get("KVX_ATDA_LPE", "")}


if __name__ == "__main__":
    _lib.require_device()
    print(json.dumps({"digest": digest, "atda": atda}[sys.argv[1]](), sort_keys=True))
