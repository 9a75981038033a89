"""The interior-point loop of coneqp (_ipm.coneqp_loop) on the host: a numpy engine with dense P, G, p = 0 and the KKT solve by
numpy.linalg.solve on S = P + G' di^2 G stands in for the device engines, so the host logic that picks "optimal" or "unknown", and
the ValueError of a rank-deficient problem, runs without a GPU.  Compared with the reference's own run in tests/golden/g5_coneqp.*
(6x5 grid) to 1e-10 relative.  Measured: the scaling d of the first six factorisations differs from the reference's by 4.5e-16 to
4.9e-15, more than a thousand times below the bound; the returned x differs by 1.35e-12, only 74 times below it.  That is the
conditioning of the problem, not the loop: cond(S) grows from 3.8 to 3.7e8 over the eight iterations (d of the last two differs by
1.0e-13 and 2.1e-12), and the same engine with a Cholesky solve of S in place of numpy.linalg.solve moves x by 6.8e-13.  The bound
stays 1e-10 for both."""
import json
import os

import numpy as np
import pytest

from kvxopt_amd import _ipm, workloads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class NumpyQpEngine:
    """_ipm.coneqp_loop's engine protocol in numpy.  KKT solve (misc.py:1489-1563 with p = 0 and H = P): x += G' di^2 z; x = S^-1 x;
    z = di (G x) - di z."""

    def __init__(self, P, q, G, h):
        self.P, self.q, self.G, self.h = (np.asarray(a, dtype=float) for a in (P, q, G, h))
        self.d = self.di = np.ones(len(self.h))
        self.factored, self.corrections, self.d_at_factor = 0, [], []
        # starting point (coneprog.py:2044-2105): W = I, [P G'; G -I][x; z] = [-q; h], s = -z, both pushed into the cone
        self.S = self.P + self.G.T @ self.G
        self.x, z = self.ksolve(-self.q, self.h)
        self.s, self.z = (v + (1.0 + max(-v)) if max(-v) >= -1e-8 * max(np.linalg.norm(v), 1.0) else v for v in (-z, z))

    def ksolve(self, x, z):
        x = np.linalg.solve(self.S, x + self.G.T @ (self.di * (self.di * z)))
        return x, self.di * (self.G @ x) - self.di * z

    def stats(self):
        Pxq = self.P @ self.x + self.q
        self.rx = Pxq + self.G.T @ self.z
        self.rz = self.s + self.G @ self.x - self.h
        return self.x @ Pxq, self.x @ self.q, self.rx @ self.rx, 0.0, self.rz @ self.rz, 0.0, self.z @ self.rz

    def scaling(self):
        self.d = np.sqrt(self.s / self.z)
        self.di = 1.0 / self.d
        self.lmbda = np.sqrt(self.s * self.z)

    def factor(self):
        self.factored += 1
        self.d_at_factor.append(self.d)
        self.S = self.P + self.G.T @ ((self.di ** 2)[:, None] * self.G)

    def direction(self, i, sigma_mu, eta, correction):
        self.corrections.append(correction)
        ds = -self.lmbda ** 2 + sigma_mu                 # right-hand side (coneprog.py:2367-2390), then f4_no_ir (:2283-2313)
        if correction and i == 1:
            ds = ds - self.ws3
        ds = ds / self.lmbda
        self.dx, dz = self.ksolve((-1.0 + eta) * self.rx, (-1.0 + eta) * self.rz - self.d * ds)
        ds = ds - dz
        dsdz = ds @ dz
        if correction and i == 0:
            self.ws3 = ds * dz
        self.ds, self.dz = ds / self.lmbda, dz / self.lmbda
        return dsdz, max(-self.ds), max(-self.dz)

    def update(self, step):
        self.x = self.x + step * self.dx
        rs, rz = (np.sqrt((1.0 + step * v) * self.lmbda) for v in (self.ds, self.dz))       # misc.py:444-464
        self.d = self.d * rs / rz
        self.di = 1.0 / self.d
        self.lmbda = rs * rz
        self.s, self.z = self.d * self.lmbda, self.di * self.lmbda
        return self.lmbda @ self.lmbda


@pytest.fixture(scope="module")
def qp():
    Q = workloads.qp_grid(6, 5)
    n, cols = Q["n"], np.repeat(np.arange(Q["n"]), np.diff(Q["Gp"]))
    G = np.zeros((Q["ml"], n))
    G[Q["Gi"], cols] = Q["Gx"]
    P = np.zeros((n, n))
    P[Q["Pi"], np.repeat(np.arange(n), np.diff(Q["Pp"]))] = Q["Px"]
    return P + np.tril(P, -1).T, Q["q"], G, Q["h"]


def run(qp, options=None, engine=NumpyQpEngine):
    e = engine(*qp)
    res0 = (max(1.0, np.linalg.norm(e.q)), 1.0, max(1.0, np.linalg.norm(e.h)))
    return e, _ipm.coneqp_loop(e, _ipm.options(options, {}, qp=True), len(e.h), e.s @ e.z, res0)


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / np.abs(b).max()


def test_loop_grid6x5(qp):
    meta = json.load(open(os.path.join(GOLDEN, "g5_coneqp.json")))["cases"]["qp6x5"]
    e, out = run(qp)
    assert out.status == meta["status"] == "optimal" and out.msg is None
    assert out.iterations == meta["iterations"] == 8 and e.factored == 8
    g = np.load(os.path.join(GOLDEN, "g5_coneqp.npz"))
    errs = [rel(d, dg) for d, dg in zip(e.d_at_factor, g["qp6x5_d_per_iter"])] + [rel(e.x, g["qp6x5_x"])]
    print("relative distance to the golden of d per iteration, then of x: " + " ".join("%.2e" % v for v in errs))
    assert len(errs) == 9 and max(errs) < 1e-10
    assert e.corrections == [True] * 16
    gap, relgap, pcost, dcost, pres, dres = out.stats
    assert abs(pcost - meta["primal objective"]) < 1e-10 * abs(meta["primal objective"]) and pres <= 1e-7 and dres <= 1e-7


def test_loop_maxiters(qp):
    e, out = run(qp, {"maxiters": 2})
    assert (out.status, out.iterations, out.msg) == ("unknown", 2, _ipm.MAXITERS_MSG)
    assert e.factored == 2 and None not in out.stats[:1] + out.stats[2:]


@pytest.mark.parametrize("method", ["factor", "direction"])
def test_loop_singular_kkt(qp, method):
    def failing(at):
        class Singular(NumpyQpEngine):
            calls = 0

            def fail(self, *args):
                self.calls += 1
                if self.calls == at:
                    raise ArithmeticError("singular")
                return getattr(NumpyQpEngine, method)(self, *args)
        setattr(Singular, method, Singular.fail)
        return Singular

    # the second factorisation, or the first solve of the second iteration: the iterates of the first iteration are returned
    e, out = run(qp, engine=failing(2 if method == "factor" else 3))
    assert (out.status, out.iterations, out.msg) == ("unknown", 1, _ipm.SINGULAR_MSG)
    assert len(out.stats) == 6 and out.stats[0] > 0.0
    with pytest.raises(ValueError, match="Rank"):                       # at the first iteration: the problem, not the iterate
        run(qp, engine=failing(1))


def test_loop_without_correction(qp):
    """use_correction False: no direction is asked for the Mehrotra term, and the loop still ends at the same optimum -- both
    objectives lie within the gap of it, which the exit test bounds by reltol = 1e-6 of the objective (asserted with a factor 10)."""
    meta = json.load(open(os.path.join(GOLDEN, "g5_coneqp.json")))["cases"]["qp6x5"]
    e, out = run(qp, {"use_correction": False})
    assert out.status == "optimal" and e.corrections == [False] * (2 * out.iterations) and not hasattr(e, "ws3")
    gap, relgap, pcost, dcost, pres, dres = out.stats
    assert pres <= 1e-7 and dres <= 1e-7 and (gap <= 1e-7 or relgap <= 1e-6)
    assert abs(pcost - meta["primal objective"]) <= 1e-5 * max(1.0, abs(meta["primal objective"]))
