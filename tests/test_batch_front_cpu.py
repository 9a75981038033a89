"""Which check wins when a call to the batch family breaks two or more of them at once: the Python text for the seven _prepare
functions and the four derivative entries, the return code and kvx_last_error for every kvx_*_batch_solve[_dev],
kvx_{qp,coneqp}_batch_{vjp,jvp}[_dev] and the two *_diff_lds_bytes queries.  Every check runs before a device is asked for and every
case here is refused, so nothing is launched, with or without a device.  The expected answers (golden/batch_front.json) were
recorded by running this file as a program (`python tests/test_batch_front_cpu.py` prints the table as JSON) on the commit before
the checks were gathered in kvxopt_amd/_batch.py and csrc/batch_cone_host.hpp; they hold every later change of the front to the
same order and the same texts."""
import json
import os

import numpy as np
import pytest

from kvxopt_amd import _lib, conelpbatch, coneqpbatch, gpbatch, lpbatch, qpbatch, sdpbatch, socpbatch, solvers

CASES = {}
REF = {"refinement": 1}
ONES = np.ones


# ---- Python: the seven _prepare functions under one set of names
DIMS = {"socp": {"l": 1, "q": []}, "sdp": {"l": 1, "s": []}, "conelp": {"l": 1, "q": [], "s": []}, "coneqp": {"l": 1, "q": [], "s": []}}
FRONTS = ("qp", "lp", "socp", "sdp", "conelp", "coneqp", "gp")


def front(name, n=2, lin=None, G=None, h=None, dims=None, A=None, b=None, options=None, K=None, F=None, P=None):
    """_prepare of one entry on a batch of two members with n variables and one 'l' row unless told otherwise."""
    G = ONES((1, n)) if G is None else G
    h = ONES(1) if h is None else h
    dims = DIMS.get(name) if dims is None else dims
    P = np.eye(n) if P is None else P
    if name == "gp":
        F = ONES((1, n)) if F is None else F
        lin = ONES((1, 2)) if lin is None else lin
        return gpbatch._prepare([1] if K is None else K, F, lin, G, h, A, b, options)
    lin = ONES((n, 2)) if lin is None else lin
    if name == "qp":
        return qpbatch._prepare(P, lin, G, h, A, b, options)
    if name == "lp":
        return lpbatch._prepare(lin, G, h, A, b, options)
    if name == "coneqp":
        return coneqpbatch._prepare(P, lin, G, h, dims, A, b, options)
    return {"socp": socpbatch, "sdp": sdpbatch, "conelp": conelpbatch}[name]._prepare(lin, G, h, dims, A, b, options)


def py(name, what, **kw):
    CASES["py/%s/%s" % (name, what)] = lambda: front(name, **kw)


for f in FRONTS:
    py(f, "refinement+p>n", options=REF, A=ONES((3, 2)))
    py(f, "refinement+maxiters=0", options={"refinement": 1, "maxiters": 0})
    py(f, "maxiters=0+h-rows", options={"maxiters": 0}, h=ONES(2))
    py(f, "p>n+b-absent", A=ONES((3, 2)))
    py(f, "A+b-absent+rank", n=3, A=ONES((1, 3)))
    py(f, "A-absent+b-given+rank", n=3, b=ONES(1))
    py(f, "h-rows+b-absent", h=ONES(2), A=ONES((1, 2)))
    py(f, "G-members+h-columns", G=ONES((3, 1, 2)), h=ONES((1, 3)))
    py(f, "A-members+b-columns", A=ONES((3, 1, 2)), b=ONES((1, 3)))
    py(f, "A-columns+b-absent", A=ONES((1, 3)))
    py(f, "b-rows+rank", n=3, A=ONES((1, 3)), b=ONES(2))
    py(f, "p=0-A-given+b-given", A=np.zeros((0, 2)), b=ONES(1))
    if f != "gp":
        py(f, "no-members+n=0", lin=np.zeros((0, 0)))
        py(f, "n=0+p>n", lin=np.zeros((0, 2)), G=ONES((1, 0)), A=ONES((1, 0)))
for f in ("qp", "lp"):
    py(f, "n=0+ml=0", lin=np.zeros((0, 2)), G=np.zeros((0, 0)))
    py(f, "refinement+ml=0", options=REF, G=np.zeros((0, 2)))
    py(f, "ml=0+p>n", G=np.zeros((0, 2)), A=ONES((3, 2)))
for f in ("qp", "coneqp"):
    py(f, "P-rows+G-columns", P=np.eye(3), G=ONES((1, 3)))
    py(f, "P-members+n=0", lin=np.zeros((0, 2)), P=np.zeros((3, 0, 0)))
for f in ("socp", "conelp", "coneqp"):
    py(f, "n=0+nq=129", lin=np.zeros((0, 2)), dims=dict(DIMS[f], q=[1] * 129))
    py(f, "nq=129+N>limit", dims=dict(DIMS[f], l=400, q=[1] * 129))
    py(f, "refinement+N=0", options=REF, dims=dict(DIMS[f], l=0))
for f in ("sdp", "conelp", "coneqp"):
    py(f, "n=0+ns=33", lin=np.zeros((0, 2)), dims=dict(DIMS[f], s=[1] * 33))
    py(f, "m_k=17+N>384", dims=dict(DIMS[f], s=[17, 17]))
    py(f, "ns=33+m_k=17", dims=dict(DIMS[f], s=[17] * 33))
    py(f, "N>384+G-rows", dims=dict(DIMS[f], l=385))
for f in ("socp", "sdp", "conelp", "coneqp"):
    py(f, "dims-not-a-dict+refinement", dims=[1], options=REF)
    py(f, "dims-negative-l+refinement", dims=dict(DIMS[f], l=-1), options=REF)
    py(f, "G-rows+h-rows", G=ONES((2, 2)), h=ONES(3))
    py(f, "N=0+p>n", dims=dict(DIMS[f], l=0), A=ONES((3, 2)))
py("socp", "refinement+dims-s", options=REF, dims={"l": 1, "q": [], "s": [2]})
py("socp", "dims-s+n=0", lin=np.zeros((0, 2)), dims={"l": 1, "q": [], "s": [2]})
py("sdp", "refinement+dims-q", options=REF, dims={"l": 1, "q": [2], "s": []})
py("sdp", "dims-q+n=0", lin=np.zeros((0, 2)), dims={"l": 1, "q": [2], "s": []})
py("conelp", "N>384-without-s+p>n", dims={"l": 385, "q": [], "s": []}, A=ONES((3, 2)))
py("conelp", "N>384-with-s+p>n", dims={"l": 384, "q": [], "s": [1]}, A=ONES((3, 2)))
py("gp", "K-not-a-list+F-rows", K=(1,), F=ONES((2, 2)))
py("gp", "F-rows+g-rows", F=ONES((2, 2)), lin=ONES((2, 2)))
py("gp", "g-rows+no-members", lin=np.zeros((2, 0)))
py("gp", "F-float32+A-columns", F=ONES((1, 2), dtype=np.float32), A=ONES((1, 3)))
py("gp", "G-columns+n=0", F=ONES((1, 0)), G=ONES((1, 2)))
py("gp", "n=0+p>n", F=ONES((1, 0)), G=ONES((1, 0)), A=ONES((1, 0)))
py("gp", "h-absent+b-absent", A=ONES((1, 2)), h=None, G=ONES((2, 2)))
py("gp", "h-rows+p>n", h=ONES(2), A=ONES((3, 2)))
py("gp", "N>192+p>n", K=[1] * 193, F=ONES((193, 2)), lin=ONES((193, 2)), A=ONES((3, 2)))
py("gp", "refinement+K-empty", options=REF, K=[])


# ---- Python: the four derivative entries
def derivative(name, n=2, N=1, p=0, A=None, b=None, sol=0, **kw):
    P, q, G, h = np.eye(n), ONES((n, 2)), ONES((N, n)), ONES(N)
    if sol == 0:
        sol = {"x": ONES((n, 2)), "y": ONES((p, 2)), "s": ONES((N, 2)), "z": ONES((N, 2)), "exit": np.zeros(2, dtype=np.int64)}
    if "vjp" in name:
        kw.setdefault("gx", ONES((n, 2)))
    fn = getattr(solvers, name)
    if name.startswith("coneqp"):
        return fn(P, q, G, h, {"l": N, "q": [], "s": []}, A, b, sol=sol, **kw)
    return fn(P, q, G, h, A, b, sol=sol, **kw)


def pyd(name, what, **kw):
    CASES["py/%s/%s" % (name, what)] = lambda: derivative(name, **kw)


GOOD = {"x": ONES((2, 2)), "y": ONES((0, 2)), "s": ONES((1, 2)), "z": ONES((1, 2)), "exit": np.zeros(2, dtype=np.int64)}
for f in ("qp_batch_vjp", "qp_batch_jvp", "coneqp_batch_vjp", "coneqp_batch_jvp"):
    pyd(f, "refinement=4+p>n", options={"refinement": 4}, A=ONES((3, 2)))
    pyd(f, "unknown-option+refinement=-1", options={"maxiters": 1, "refinement": -1})
    pyd(f, "refinement-bool+sol-absent", options={"refinement": True}, sol=None)
    pyd(f, "p>n+sol-absent", A=ONES((3, 2)), sol=None)
    pyd(f, "N=0+sol-absent", N=0, sol=None)
    pyd(f, "b-absent+sol-absent", A=ONES((1, 2)), sol=None)
    pyd(f, "sol-x-shape+sol-exit-float", sol=dict(GOOD, x=ONES((3, 2)), exit=np.zeros(2)))
    pyd(f, "sol-z-shape+sol-exit-length", sol=dict(GOOD, z=ONES((2, 2)), exit=np.zeros(3, dtype=np.int64)))
for f in ("qp_batch_vjp", "coneqp_batch_vjp"):
    pyd(f, "sol-key-missing+gx-shape", sol={"x": 1}, gx=ONES((3, 2)))
    pyd(f, "sol-exit-float+wrt", sol=dict(GOOD, exit=np.zeros(2)), wrt=("x",))
    pyd(f, "gx-shape+wrt", gx=ONES((3, 2)), wrt=("q", "x", "y"))
    pyd(f, "gx-3d+wrt", gx=ONES((2, 2, 2)), wrt="x")
for f in ("qp_batch_jvp", "coneqp_batch_jvp"):
    pyd(f, "sol-key-missing+dP-shape", sol={"x": 1}, dP=np.eye(3))
    pyd(f, "dP-shape+db-given", dP=np.eye(3), db=ONES(1))
    pyd(f, "dq-rows+dG-members", dq=ONES(3), dG=ONES((3, 1, 2)))
    pyd(f, "dG-members+dh-columns", dG=ONES((3, 1, 2)), dh=ONES((1, 3)))
    pyd(f, "dh-rows+dA-given", dh=ONES(2), dA=ONES((1, 2)))
    pyd(f, "dA-given+db-given", dA=ONES((1, 2)), db=ONES(1))
for f in ("coneqp_batch_vjp", "coneqp_batch_jvp"):
    pyd(f, "refinement=4+centering=17", options={"refinement": 4, "centering": 17})
    pyd(f, "centering=17+centol=0", options={"centering": 17, "centol": 0.0})
    pyd(f, "centering-float+refinement=4", options={"centering": 1.5, "refinement": 4})
    pyd(f, "centol=0+p>n", options={"centol": 0.0}, A=ONES((3, 2)))
    pyd(f, "unknown-option+centol-text", options={"abstol": 1.0, "centol": "tight"})


# ---- C: kvx_*_batch_solve and kvx_*_batch_solve_dev
BUF, INTS = np.zeros(64), np.zeros(8, dtype=np.int64)
DATA = {"qp": "PqGhAb", "coneqp": "PqGhAb", "gp": "FgGhAb"}


def pointers(dev):
    return ((lambda a: a.ctypes.data), (lambda a: a.ctypes.data)) if dev else (_lib.pd, _lib.pi)


def c_solve(entry, B=2, n=2, ml=1, p=0, q=(), m=(), K=(1,), nullq=False, nullm=False, nullK=False, strides=None, null=(), maxiters=10,
            abstol=1e-7, reltol=1e-6, feastol=1e-7):
    """One call of a solve entry on small valid arguments except for what the case names; null: the names of NULL pointers."""
    fam, dev = entry.split("_")[1], entry.endswith("_dev")
    D, Di = pointers(dev)
    qv, mv, Kv = (np.asarray(v, dtype=np.int64) for v in (q, m, K))
    qa, ma = [len(q), None if nullq or not q else _lib.pi(qv)], [len(m), None if nullm or not m else _lib.pi(mv)]
    args = {"qp": [B, n, ml, p], "lp": [B, n, ml, p], "socp": [B, n, ml] + qa + [p], "sdp": [B, n, ml] + ma + [p],
            "conelp": [B, n, ml] + qa + ma + [p], "coneqp": [B, n, ml] + qa + ma + [p],
            "gp": [B, n, len(K) - 1, None if nullK else _lib.pi(Kv), ml, p]}[fam]
    for name in DATA.get(fam, "cGhAb"):
        args += [None if name in null else D(BUF), (strides or {}).get(name, 0)]
    args += [maxiters, abstol, reltol, feastol] + ([1] if fam in ("qp", "coneqp") else [])
    args += [None if name in null else D(BUF) for name in ("x", "y", "s", "z", "stats")]
    args += [None if name in null else Di(INTS) for name in ("iterations", "exit")]
    if fam == "gp" and dev:
        args.append(None if "scratch" in null else D(BUF))
    rc = getattr(_lib.lib(), entry)(*args)
    return "%d: %s" % (rc, _lib.last_error())


def c(entry, what, **kw):
    CASES["c/%s/%s" % (entry, what)] = lambda: c_solve(entry, **kw)


for fam in FRONTS:
    lin = DATA.get(fam, "cGhAb")[1 if fam in DATA else 0]
    for entry in ("kvx_%s_batch_solve" % fam, "kvx_%s_batch_solve_dev" % fam):
        c(entry, "B=0+n=0", B=0, n=0)
        c(entry, "n=65+p=-1", n=65, p=-1)
        c(entry, "p>n+linear-NULL", p=3, null=(lin,))
        c(entry, "p>n+maxiters=0", p=3, maxiters=0)
        c(entry, "A-NULL+x-NULL", p=1, null=("A", "x"))
        c(entry, "b-NULL+y-NULL", p=1, null=("b", "y"))
        c(entry, "exit-NULL+G-stride", null=("exit",), strides={"G": 1})
        c(entry, "G-stride+maxiters=0", strides={"G": 1}, maxiters=0)
        c(entry, "linear-stride+h-stride", strides={lin: 1, "h": -1})
        c(entry, "A-stride+feastol=0", p=1, strides={"A": 1}, feastol=0.0)
        c(entry, "maxiters=0+feastol=0", maxiters=0, feastol=0.0)
        c(entry, "feastol=nan+tolerances", feastol=float("nan"), abstol=0.0, reltol=-1.0)
        c(entry, "n-beyond-int32+ml=-1", n=2 ** 40, ml=-1)
        if fam in ("qp", "lp"):
            c(entry, "n=65+ml=0", n=65, ml=0)
            c(entry, "ml=513+p>n", ml=513, p=3)
            c(entry, "ml=0+G-NULL", ml=0, null=("G",))
        if fam in ("qp", "coneqp"):
            c(entry, "P-NULL+stats-NULL", null=("P", "stats"))
            c(entry, "P-stride+q-stride", strides={"P": 3, "q": 1})
        if fam in ("socp", "conelp", "coneqp"):
            top = 512 if fam == "socp" else 384
            c(entry, "n=0+nq=129", n=0, q=(1,) * 129)
            c(entry, "ml>limit+nq=129", ml=top + 1, q=(1,) * 129)
            c(entry, "nq=129+q-NULL", q=(1,) * 129, nullq=True)
            c(entry, "q-NULL+p>n", q=(1,), nullq=True, p=3)
            c(entry, "order=0+N>limit", ml=top, q=(0, 1))
            c(entry, "order>limit+N>limit", ml=0, q=(top + 1,))
            c(entry, "N>limit+p>n", ml=top, q=(1,), p=3)
        if fam in ("sdp", "conelp", "coneqp"):
            c(entry, "n=0+ns=33", n=0, m=(1,) * 33)
            c(entry, "ns=33+m-NULL", m=(1,) * 33, nullm=True)
            c(entry, "m-NULL+p>n", m=(1,), nullm=True, p=3)
            c(entry, "order=17+N>384", ml=384, m=(17,))
            c(entry, "order=0+p>n", m=(0,), p=3)
            c(entry, "N>384+p>n", ml=384, m=(1,), p=3)
        if fam in ("conelp", "coneqp"):
            c(entry, "q-NULL+ns=33", q=(1,), nullq=True, m=(1,) * 33)
            c(entry, "cone-order=0+block-order=17", q=(0,), m=(17,))
            c(entry, "N=0+p>n", ml=0, p=3)
        if fam in ("lp", "socp", "sdp", "conelp"):
            c(entry, "rank+linear-NULL", n=3, null=(lin,))
            c(entry, "p>n+rank", n=3, p=4)
        if fam == "gp":
            c(entry, "n=64+K-NULL", n=64, nullK=True)
            c(entry, "K-NULL+ml=-1", nullK=True, ml=-1)
            c(entry, "K=0+N>192", K=(0,), ml=192)
            c(entry, "K>768+p>n", K=(769,), p=3)
            c(entry, "l>768+ml=-1", K=(500, 500), ml=-1)
            c(entry, "ml=-1+p>n", ml=-1, p=3)
            c(entry, "N>192+p>n", ml=192, p=3)
            c(entry, "F-NULL+F-stride", null=("F",), strides={"F": 1})
            c(entry, "G-NULL+x-NULL", null=("G", "x"))
            c(entry, "x-NULL+scratch-NULL", null=("x", "scratch"))
            c(entry, "scratch-NULL+g-stride+maxiters=0", null=("scratch",), strides={"g": -1}, maxiters=0)


# ---- C: the derivative entries
def c_diff(entry, B=2, n=2, ml=1, p=0, q=(), m=(), nullq=False, nullm=False, strides=None, null=(), refinement=1, centering=8, centol=1e-6):
    """null: names among P q G h A b | x y s z exitcode | gx gP gG gA | dP .. db | ux uy uz us | centrality steps gexit"""
    cone, dev, jvp = "coneqp" in entry, entry.endswith("_dev"), "jvp" in entry
    D, Di = pointers(dev)
    ptr = lambda name: None if name in null else D(BUF)                                   # noqa: E731
    iptr = lambda name: None if name in null else Di(INTS)                                # noqa: E731
    stride = lambda name: (strides or {}).get(name, 0)                                    # noqa: E731
    qv, mv = np.asarray(q, dtype=np.int64), np.asarray(m, dtype=np.int64)
    args = [B, n, ml]
    if cone:
        args += [len(q), None if nullq or not q else _lib.pi(qv), len(m), None if nullm or not m else _lib.pi(mv)]
    args.append(p)
    for name in ("PqGhAb" if cone else "PGA"):
        args += [ptr(name), stride(name)]
    args += [ptr("x"), ptr("y"), ptr("s"), ptr("z"), iptr("exitcode"), refinement] + ([centering, centol] if cone else [])
    if jvp:
        for name in ("dP", "dq", "dG", "dh", "dA", "db"):
            args += [ptr(name), stride(name)]
        args += [ptr("ux"), ptr("uy"), ptr("uz"), ptr("us")]
    else:
        args += [ptr("gx"), ptr("ux"), ptr("uy"), ptr("uz"), ptr("gP"), ptr("gG"), ptr("gA")]
    if cone:
        args += [ptr("centrality"), iptr("steps")]
    args.append(iptr("gexit"))
    rc = getattr(_lib.lib(), entry)(*args)
    return "%d: %s" % (rc, _lib.last_error())


def cd(entry, what, **kw):
    CASES["c/%s/%s" % (entry, what)] = lambda: c_diff(entry, **kw)


for fam in ("qp", "coneqp"):
    for mode in ("vjp", "jvp"):
        for entry in ("kvx_%s_batch_%s" % (fam, mode), "kvx_%s_batch_%s_dev" % (fam, mode)):
            cd(entry, "B=0+n=0", B=0, n=0)
            cd(entry, "n=0+p=-1", n=0, p=-1)
            cd(entry, "ml=-1+refinement=4", ml=-1, refinement=4)
            cd(entry, "p>n+P-NULL", p=3, null=("P",))
            cd(entry, "p>n+refinement=-1", p=3, refinement=-1)
            cd(entry, "refinement=4+x-NULL", refinement=4, null=("x",))
            cd(entry, "refinement=4+P-stride", refinement=4, strides={"P": 1})
            cd(entry, "G-NULL+z-NULL", null=("G", "z"))
            cd(entry, "A-NULL+y-NULL", p=1, null=("A", "y"))
            cd(entry, "exitcode-NULL+ux-NULL", null=("exitcode", "ux"))
            cd(entry, "s-NULL+gx-NULL+us-NULL", null=("s", "gx", "us"))
            cd(entry, "gx-NULL+us-NULL+gexit-NULL", null=("gx", "us", "gexit"))
            cd(entry, "uy-NULL+A-stride", p=1, null=("uy",), strides={"A": 1})
            cd(entry, "uz-NULL+P-stride", null=("uz",), strides={"P": 1})
            cd(entry, "P-stride+G-stride", strides={"P": 3, "G": 1})
            cd(entry, "G-stride+dP-stride", strides={"G": -1, "dP": 1})
            cd(entry, "dq-stride+dh-stride", strides={"dq": 1, "dh": -2, "P": 1 if mode == "vjp" else 0})
            cd(entry, "dA-stride+db-stride", p=1, strides={"dA": 1, "db": -1, "A": 1 if mode == "vjp" else 0})
            cd(entry, "dP-NULL+dP-stride+G-stride", null=("dP",), strides={"dP": 1, "G": 1})
            cd(entry, "n-beyond-int32+ml=-1", n=2 ** 40, ml=-1)
            if fam == "qp":
                cd(entry, "ml=0+refinement=-1", ml=0, refinement=-1)
                cd(entry, "n=65+ml=513", n=65, ml=513)
                continue
            cd(entry, "n=65+nq=129", n=65, q=(1,) * 129)
            cd(entry, "nq=129+q-NULL", q=(1,) * 129, nullq=True)
            cd(entry, "q-NULL+ns=33", q=(1,), nullq=True, m=(1,) * 33)
            cd(entry, "ns=33+m-NULL", m=(1,) * 33, nullm=True)
            cd(entry, "m-NULL+refinement=4", m=(1,), nullm=True, refinement=4)
            cd(entry, "order=0+N>384", ml=384, q=(0, 1))
            cd(entry, "order=17+N>384", ml=384, m=(17,))
            cd(entry, "cone-order=0+block-order=17", q=(0,), m=(17,))
            cd(entry, "N>384+p>n", ml=384, q=(1,), p=3)
            cd(entry, "N=0+centering=17", ml=0, centering=17)
            cd(entry, "p>n+centol=0", p=3, centol=0.0)
            cd(entry, "refinement=4+centering=17", refinement=4, centering=17)
            cd(entry, "centering=17+centol=0", centering=17, centol=0.0)
            cd(entry, "centering=-1+q-data-NULL", centering=-1, null=("q",))
            cd(entry, "centol=nan+P-NULL", centol=float("nan"), null=("P",))
            cd(entry, "h-NULL+s-NULL", null=("h", "s"))
            cd(entry, "b-NULL+y-NULL", p=1, null=("b", "y"))
            cd(entry, "centrality-NULL+q-stride", null=("centrality",), strides={"q": 1})
            cd(entry, "steps-NULL+h-stride", null=("steps",), strides={"h": -1})
            cd(entry, "q-stride+b-stride", p=1, strides={"q": 1, "b": -1})


# ---- C: the two queries; `forward` is written only on success
def c_query(cone, n=2, ml=1, p=0, q=(), m=(), nullq=False, nullm=False):
    fwd = np.full(1, -7, dtype=np.int64)
    qv, mv = np.asarray(q, dtype=np.int64), np.asarray(m, dtype=np.int64)
    L = _lib.lib()
    if cone:
        r = L.kvx_coneqp_batch_diff_lds_bytes(n, ml, len(q), None if nullq or not q else _lib.pi(qv), len(m),
                                              None if nullm or not m else _lib.pi(mv), p, _lib.pi(fwd))
    else:
        r = L.kvx_qp_batch_diff_lds_bytes(n, ml, p, _lib.pi(fwd))
    return "%d, forward %d" % (r, fwd[0])


def cq(cone, what, **kw):
    CASES["c/kvx_%s_batch_diff_lds_bytes/%s" % ("coneqp" if cone else "qp", what)] = lambda: c_query(cone, **kw)


for cone in (False, True):
    cq(cone, "fits")
    cq(cone, "fits-p=n", p=2)
    cq(cone, "n=0+p=-1", n=0, p=-1)
    cq(cone, "n=65+ml=-1", n=65, ml=-1)
    cq(cone, "p>n+ml=-1", p=3, ml=-1)
    cq(cone, "n-beyond-int32", n=2 ** 40)
    cq(cone, "ml-beyond-int32", ml=2 ** 40)
    cq(cone, "p-beyond-int32", n=3, p=2 ** 32 + 1)
cq(False, "ml=0", ml=0)
cq(False, "ml=513", ml=513)
cq(True, "ml=0+cones", ml=0, q=(2,), m=(2,))
cq(True, "N=0", ml=0)
cq(True, "ml=385", ml=385)
cq(True, "nq=129+q-NULL", q=(1,) * 129, nullq=True)
cq(True, "q-NULL+ns=33", q=(1,), nullq=True, m=(1,) * 33)
cq(True, "m-NULL+p>n", m=(1,), nullm=True, p=3)
cq(True, "order=0+N>384", ml=384, q=(0, 1))
cq(True, "order=17", m=(17,))
cq(True, "N>384", ml=384, q=(1,))


def observe(fn):
    try:
        r = fn()
    except Exception as e:                                       # the type and the text are what is pinned
        return "%s: %s" % (type(e).__name__, e)
    return r if isinstance(r, str) else "returned"


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_front.json")) as _f:
    EXPECTED = json.load(_f)


def test_the_table_is_complete_and_every_call_is_refused():
    assert sorted(EXPECTED) == sorted(CASES)
    assert not [k for k, v in EXPECTED.items() if v.startswith("0: ")]
    # a _prepare may pass (A with no rows: b is not looked at); an entry that would go on to the device may not
    assert [k for k, v in EXPECTED.items() if v == "returned"] == ["py/coneqp/p=0-A-given+b-given", "py/qp/p=0-A-given+b-given"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_which_check_wins(case):
    assert observe(CASES[case]) == EXPECTED[case]


if __name__ == "__main__":
    print(json.dumps({k: observe(CASES[k]) for k in sorted(CASES)}, indent=0, sort_keys=True))
