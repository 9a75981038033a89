"""Dense numpy restatement of a kept kvxopt_amd.osqp problem ("A kept problem"): update, warm start, cold
start, the polish step and the loop of osqp.Problem.solve -- the contract the kvx_admm_update / warm_start / cold_start / polish
entry points and osqp.Problem are tested against.  It builds on osqp_numpy.Admm (imported, not edited) and shares nothing with
the package.  float64 or numpy.longdouble, as there.

The polish is written as DESIGN section 11 states it, in the eliminated form and not as a dense KKT solve:

    active: lower z - l < -y, upper u - z < y;  w = 1 / delta on active rows, 0 elsewhere;  b = l or u
    S_pol = P + delta I + A' diag(w) A
    xh = S_pol^-1 (-q + A'(w o b)),  yh = w o (A xh - b)
    refine_iter x:  e1 = -q - (P xh + A' yh),  e2 = b - A xh on active rows, 0 elsewhere,
                    dx = S_pol^-1 (e1 + A'(w o e2)),  dy = w o (A dx - e2),  xh += dx,  yh += dy
    zh = clip(A xh, l, u)
"""
import numpy as np

import osqp_numpy as R

DEFAULTS = dict(R.DEFAULTS, polish=0, delta=1e-6, polish_refine_iter=3, warm_start=1)


def rho_classes(lb, ub):
    """0: no finite bound, 1: equality (u - l < 1e-4), 2: the others -- the three values of osqp_numpy.rho_vector."""
    free = (lb <= -R.INF_FROM) & (ub >= R.INF_FROM)
    return np.where(free, 0, np.where(ub - lb < 1e-4, 1, 2))


def _rule(a, b, c, d):
    return (a and b) or (a and c) or (b and d)


def accept(rp, rd, hp, hd, margins=None):
    """The acceptance rule of the polish: (rp, rd) the loop's last residuals, (hp, hd) the polished ones.  margins (a list): the
    decision's relative distance from its threshold is appended -- the rule is made of four comparisons, hp < rp, hd < rd,
    rd < 1e-10, rp < 1e-10, and the distance is the smallest relative change of the compared numbers that turns the outcome:
    over every set of comparisons whose reversal changes it, the largest distance in the set, minimised."""
    rp, rd, hp, hd = float(rp), float(rd), float(hp), float(hd)
    tests = [hp < rp, hd < rd, rd < 1e-10, rp < 1e-10]
    out = _rule(*tests)
    if margins is not None:
        dist = [abs(hp - rp) / rp if rp > 0 else 1.0, abs(hd - rd) / rd if rd > 0 else 1.0, abs(rd - 1e-10) / 1e-10, abs(rp - 1e-10) / 1e-10]
        best = float("inf")
        for mask in range(1, 16):
            flipped = [t != bool(mask >> k & 1) for k, t in enumerate(tests)]
            if _rule(*flipped) != out:
                best = min(best, max(dist[k] for k in range(4) if mask >> k & 1))
        margins.append(best)
    return out


class Session(R.Admm):
    """An Admm whose data can be replaced and that can polish.  `stale`: the kept factor is that of S_pol."""

    def set_rho(self, rho):
        super().set_rho(rho)
        self.stale = False

    def iterate(self, k):
        if self.stale and k > 0:                        # a polish took the factor over: one counted factorisation brings S back
            self.set_rho(self.rho)
        return super().iterate(k)

    # ---- new data, scaled with the kept D, E, c ------------------------------------------------------------------------------
    def update(self, q=None, l=None, u=None):
        lb, ub = self.lb64, self.ub64
        if l is not None:
            l = np.asarray(l, dtype=np.float64)
            lb = np.where(l <= -R.INF_FROM, -R.INFTY, self.E * l)
        if u is not None:
            u = np.asarray(u, dtype=np.float64)
            ub = np.where(u >= R.INF_FROM, R.INFTY, self.E * u)
        if not np.all(lb <= ub):
            raise ValueError("l <= u does not hold")
        if q is not None:
            self.qb = np.asarray((self.c * self.D) * np.asarray(q, dtype=np.float64), dtype=self.dtype)
        changed = bool(np.any(rho_classes(lb, ub) != rho_classes(self.lb64, self.ub64)))
        self.lb64, self.ub64 = lb, ub
        self.lb, self.ub = np.asarray(lb, dtype=self.dtype), np.asarray(ub, dtype=self.dtype)
        if changed:
            self.set_rho(self.rho)
        return changed

    def warm_start(self, x=None, y=None):
        if x is not None:
            self.x = self.Dinv * np.asarray(x, dtype=self.dtype)
            self.z = self.A_(self.x)
        if y is not None:
            self.y = (self.dtype(self.c) * self.Einv) * np.asarray(y, dtype=self.dtype)
        self.dx, self.dy = np.zeros(self.n, dtype=self.dtype), np.zeros(self.m, dtype=self.dtype)

    def cold_start(self):
        z = lambda k: np.zeros(k, dtype=self.dtype)
        self.x, self.z, self.y, self.dx, self.dy = z(self.n), z(self.m), z(self.m), z(self.n), z(self.m)

    # ---- polish ------------------------------------------------------------------------------------------------------------------
    def active_set(self):
        lo = self.z - self.lb < -self.y
        up = self.ub - self.z < self.y
        assert not (lo & up).any()
        return np.where(lo, -1, np.where(up, 1, 0)).astype(np.int64)

    def polish(self, delta=1e-6, refine_iter=3):
        """The 16 numbers of kvx_admm_polish; xh, zh, yh, act are kept on the object."""
        t = self.dtype
        out = np.zeros(16, dtype=t)
        act = self.active_set()
        self.act = act
        on = act != 0
        out[1], out[2] = (act < 0).sum(), (act > 0).sum()
        w = np.where(on, t(1.0) / t(delta), t(0.0))
        b = np.where(act < 0, self.lb, np.where(act > 0, self.ub, t(0.0)))
        Spol = self.Pb + t(delta) * np.eye(self.n, dtype=t) + self.Ab.T @ (w[:, None] * self.Ab)
        self.nfact += 1
        self.stale = True
        try:
            if self.fast:
                import scipy.linalg
                fac = scipy.linalg.cho_factor(Spol, lower=True)
                solve = lambda r: scipy.linalg.cho_solve(fac, r)
            else:
                fac = R._chol(Spol)
                solve = lambda r: R._chol_solve(fac, r)
        except (np.linalg.LinAlgError, ArithmeticError):
            out[0] = -1
            self.xh = self.zh = self.yh = None
            return out
        out[0] = 1
        xh = solve(-self.qb + self.At_(w * b))
        yh = w * (self.A_(xh) - b)
        out[9], out[10] = np.abs(self.qb).max(), np.abs(b).max()
        for _ in range(refine_iter):
            e1 = -self.qb - (self.P_(xh) + self.At_(yh))
            e2 = np.where(on, b - self.A_(xh), t(0.0))
            out[9], out[10] = np.abs(e1).max(), np.abs(e2).max()
            dx = solve(e1 + self.At_(w * e2))
            dy = w * (self.A_(dx) - e2)
            xh, yh = xh + dx, yh + dy
        self.xh, self.yh = xh, yh
        self.zh = np.minimum(np.maximum(self.A_(xh), self.lb), self.ub)
        out[3:9] = self.polish_numbers(xh, yh)[0]
        return out

    def polish_numbers(self, xh, yh):
        """out[3:9] of kvx_admm_polish at the given scaled (xh, yh), and the scale of each: for the four residuals the largest
        infinity norm among the vectors the residual is the sum of (they cancel), for the two sums the sum of the absolute
        values of their terms."""
        t = self.dtype
        xh, yh = np.asarray(xh, dtype=t), np.asarray(yh, dtype=t)
        nrm = lambda v: np.abs(v).max()
        ax, px, aty = self.A_(xh), self.P_(xh), self.At_(yh)
        zh = np.minimum(np.maximum(ax, self.lb), self.ub)
        rd = px + self.qb + aty
        s = self.Dinv * self.cinv
        v = np.array([nrm(ax - zh), nrm(rd), nrm(self.Einv * (ax - zh)), nrm(rd * s), xh @ px, self.qb @ xh], dtype=t)
        scale = [max(nrm(ax), nrm(zh)), max(nrm(px), nrm(aty), nrm(self.qb)), max(nrm(self.Einv * ax), nrm(self.Einv * zh)),
                 max(nrm(px * s), nrm(aty * s), nrm(self.qb * s)), np.abs(xh) @ (np.abs(self.Pb) @ np.abs(xh)), np.abs(self.qb) @ np.abs(xh)]
        return v, [float(c) for c in scale]

    def polish_accept(self):
        self.x, self.z, self.y = self.xh.copy(), self.zh.copy(), self.yh.copy()
        self.dx, self.dy = np.zeros(self.n, dtype=self.dtype), np.zeros(self.m, dtype=self.dtype)

    def solution(self, kind=0):
        if kind == 3:
            return self.Dv * self.xh, self.Ev * self.yh * self.cinv
        return super().solution(kind)


def settings(opts):
    o = dict(DEFAULTS)
    o.update({k: v for k, v in (opts or {}).items() if k in DEFAULTS})
    return o


def new_session(p, opts=None, dtype=np.float64):
    o = settings(opts)
    return Session(p["P"], p["q"], p["A"], p["l"], p["u"], int(o["scaling"]), o["sigma"], o["rho"], o["alpha"], dtype)


def session_solve(S, opts=None, margins=None, polish_margins=None):
    """osqp.Problem.solve on a Session: (status, x, y, info)."""
    o = settings(opts)
    if not o["warm_start"]:
        S.cold_start()
    status, it = R.run(S, o, margins)
    res = S.residuals()
    b = 0 if o["scaled_termination"] else 7
    info = {"iterations": it, "status_polish": 0, "pri_res": float(res[b]), "dua_res": float(res[b + 3]), "pri_res_polish": None,
            "dua_res_polish": None, "obj_val": float((0.5 * res[22] + res[23]) * S.cinv), "active_lower": None, "active_upper": None}
    kind = 0 if status.startswith("solved") else 1 if status.startswith("primal") else 2 if status.startswith("dual") else None
    if o["polish"] and status == "solved":
        out = S.polish(o["delta"], int(o["polish_refine_iter"]))
        info["active_lower"], info["active_upper"] = int(out[1]), int(out[2])
        info["status_polish"] = -1
        if out[0] > 0:
            hp, hd = (out[3], out[4]) if o["scaled_termination"] else (out[5], out[6])
            info["pri_res_polish"], info["dua_res_polish"] = float(hp), float(hd)
            if accept(res[b], res[b + 3], hp, hd, polish_margins):
                S.polish_accept()
                info["status_polish"] = 1
                info["obj_val"] = float((0.5 * out[7] + out[8]) * S.cinv)
                kind = 3
    x, y = S.solution(kind) if kind is not None else (np.zeros(S.n), np.zeros(S.m))
    info["factorisations"] = S.nfact
    return status, np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), info
