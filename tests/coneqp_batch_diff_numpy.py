"""The restatement kvxopt_amd.coneqpbatchdiff is tested against, built on coneqp_batch_numpy.ConeqpEngine.  For one member of a
batch from coneqp_batch_numpy.members and a given x, y, s, z it has, in float64 or numpy.longdouble,

  the point      the Nesterov-Todd scaling from s and z (misc.compute_scaling), then at most `centering` centring steps: a Newton
                 step of coneqp with sigma = 1, no Mehrotra term and mu = s'z / degree of the incoming point, the full residuals on
                 the right-hand side, the step length min(1, 0.99 / t), misc.update_scaling; stopped as soon as
                 |lmbda o lmbda - mu e|_2 <= centol mu
  the system     K = [P A' G'; A 0 0; G 0 -W'W] at the centred point: the reduced solve of the engine with `refinement` steps on the
                 residual of the full system as csrc/coneqp_batch_diff.hip does it ('reduced', float64), or a dense elimination
                 (qp_batch_diff_numpy.eliminate) on the packed rows of the cone in the scaled unknown W uz, in the engine's dtype
  the outputs    the right-hand sides of both modes, the gradient formulas on full symmetric 's' blocks, ds = -W'W dz,

and for a whole batch the per-member and summed gradients, the exit codes, 'centrality' and 'centering steps' in the layout of
coneqp_batch_vjp / coneqp_batch_jvp.  Also the batches of tests/test_coneqp_batch_diff_gpu.py and the table of DESIGN section 21."""
import copy
import functools
import types

import numpy as np

import conelp_batch_numpy as CLN
import coneqp_batch_numpy as CQN
import qp_batch_diff_numpy as QDN
import sdp_batch_numpy as SDN
from kvxopt_amd import _ipm

NAMES = QDN.NAMES
rule, eliminate, inner_plain = QDN.rule, QDN.eliminate, QDN.inner
EXIT_DONE, EXIT_SKIPPED, EXIT_FAILED, EXIT_NOT_CENTRED = range(4)
SOLVE_TOL = {"abstol": 1e-8, "reltol": 1e-8, "feastol": 1e-8}

# ---- the batches: name -> (shape, B, seed, rank of P or None).  A seed may be changed, never a bound.  One was:
# "p-zero" (951 -> 954).  A cone LP solved to 1e-8 ends at a vertex, where S = Gs'Gs is nearly singular, and float64 loses a pivot of
# it in the solve or in a centring step on 7, 2, 3, 1, 3, 3, 3, 0 of the twelve members at the seeds 951 .. 958; one of twelve is allowed.
SHAPES, CORNER, EDGE, shape_name = CLN.SHAPES, CLN.CORNER, CLN.EDGE, CLN.shape_name
NO_QS, NO_S, NO_Q = CLN.NO_QS, CLN.NO_S, CLN.NO_Q
MANY = (12, 3, (2,) * 6, (1, 2, 3), 2)
BATCHES = {shape_name(s): (s, 12, 901 + k, None) for k, s in enumerate(SHAPES)}
BATCHES.update({
    "absent-qs": (NO_QS, 12, 921, None),
    "absent-s": (NO_S, 12, 922, None),
    "absent-q": (NO_Q, 12, 923, None),
    "independence": (EDGE, 300, 931, None),
    "mixed": (EDGE, 12, 941, None),
    "p-zero": (EDGE, 12, 954, 0),
})
SMALL_BATCHES = sorted(k for k in BATCHES if k != "independence")
# The batch of mixed outcomes: EDGE with the P of member 0 for all members, solved with maxiters = 6 at the default tolerances of
# coneqp_batch.  In the restatement 1, 1, 0, 3 of the twelve members are done by then at the seeds 941 .. 944; the test needs two.
MIXED_OUTCOMES = (EDGE, 12, 944)
FD_BATCHES = ("independence", "absent-q", "absent-s", shape_name(SHAPES[1]), shape_name(MANY))
FD_MEMBERS = 12                               # of "independence" the first twelve
EPS = 1e-4
TIGHT_LONGDOUBLE = {"abstol": 1e-10, "reltol": 1e-10, "feastol": 1e-10}


@functools.lru_cache(maxsize=None)
def batch(name):
    (n, ml, q, s, p), B, seed, rank = BATCHES[name]
    return CQN.members(n, ml, q, s, p, B, seed, rank)


@functools.lru_cache(maxsize=None)
def mixed_outcomes():
    (n, ml, q, s, p), B, seed = MIXED_OUTCOMES
    M = CQN.members(n, ml, q, s, p, B, seed)
    M.P = np.ascontiguousarray(np.broadcast_to(M.P[0], M.P.shape))
    return M


@functools.lru_cache(maxsize=None)
def solved(name, precision="float64"):
    """The restated solutions of batch(name) at SOLVE_TOL as the dictionary coneqp_batch returns; computed once, left unchanged."""
    return solution(CQN.restate(batch(name), SOLVE_TOL, getattr(np, precision)))


def solution(ref):
    stack = lambda name: np.stack([getattr(r, name) for r in ref], axis=1)              # noqa: E731
    return {"x": stack("x"), "y": stack("y"), "s": stack("s"), "z": stack("z"), "exit": np.array([r.exit for r in ref], dtype=np.int64)}


# ---- one member
def degree(e):
    return e.ml + len(e.q) + sum(e.sd)


def centrality(e, mu):
    """|lmbda o lmbda - mu e|_2 / mu: the Jordan product on the 'l' and 'q' rows, lmbda_k^2 - mu on the diagonal of a block."""
    v = e.lam_sq() - e.e(mu)
    return float(np.sqrt(v @ v) / mu)


def _finite(e):
    parts = [e.lmbda.a, e.d, e.di] + list(e.v) + [np.asarray(e.beta, dtype=e.t)] + list(e.r) + list(e.rti)
    return all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in parts)


def place(M, k, sol, dtype):
    """The engine of member k at the point of `sol` with its scaling: (engine, exit code 0 or 2)."""
    e = CQN.ConeqpEngine(*CQN.member(M, k), dtype)
    for v, name in ((e.x, "x"), (e.y, "y"), (e.s, "s"), (e.z, "z")):
        v.a = np.asarray(sol[name][:, k], dtype=dtype).copy()
    s, z = e.s.a[:e.ml], e.z.a[:e.ml]
    if not np.all((s > 0) & np.isfinite(s) & (z > 0) & np.isfinite(z)):
        return e, EXIT_FAILED
    try:
        with np.errstate(all="ignore"):
            e.scaling()
    except (ArithmeticError, ValueError, np.linalg.LinAlgError):
        return e, EXIT_FAILED
    return e, (EXIT_DONE if _finite(e) else EXIT_FAILED)


def centring_step(e, mu):
    """One centring step in place.  ArithmeticError when a pivot fails."""
    e.stats()
    e.factor()
    _, ts, tz = e.direction(1, mu, 0.0, False)
    e.update(_ipm.step_length(max(0.0, ts, tz), 1))


def trajectory(M, k, sol, dtype, cap, centol):
    """The states of member k after 0, 1, ... centring steps, until the threshold is met or `cap` steps are taken: a list of
    (engine, centrality) whose engines are independent copies, and the exit code of what ended it early (0 or 2).  The run with
    a smaller cap is a prefix of this one."""
    e, code = place(M, k, sol, dtype)
    if code:
        return [], code
    mu = (e.s.a @ e.z.a) / degree(e)
    out = [(copy.deepcopy(e), centrality(e, mu))]
    while len(out) <= cap and not out[-1][1] <= centol:
        try:
            with np.errstate(all="ignore"):
                centring_step(e, mu)
        except (ArithmeticError, ValueError, np.linalg.LinAlgError):
            return out, EXIT_FAILED
        out.append((copy.deepcopy(e), centrality(e, mu)))
    return out, EXIT_DONE


def centred(traj, code, centering, centol):
    """(engine, exit, centrality, steps) of the run with the cap `centering` from its trajectory; the engine is factored at the
    centred point.  centering = 0 takes the point as it is."""
    if not traj:
        return None, code, np.nan, 0
    steps = min(centering, len(traj) - 1)
    if code and steps == len(traj) - 1 and not traj[-1][1] <= centol and centering > steps:
        return None, EXIT_FAILED, np.nan, steps                      # the step after the last state failed
    e, cen = traj[steps]
    if centering > 0 and not cen <= centol:
        return None, EXIT_NOT_CENTRED, cen, steps
    e = copy.deepcopy(e)
    try:
        e.factor()
    except (ArithmeticError, ValueError, np.linalg.LinAlgError):
        return None, EXIT_FAILED, np.nan, steps
    return e, EXIT_DONE, cen, steps


def packed(e):
    """(rows, mirror rows, weights) of the packed rows of the cone: the 'l' and 'q' rows, then the lower triangle of every block."""
    rows, mir = list(range(e.Ms)), list(range(e.Ms))
    for _, o, _, m in e.blk:
        for j in range(m):
            for i in range(j, m):
                rows.append(o + i + j * m)
                mir.append(o + j + i * m)
    rows, mir = np.array(rows, dtype=int), np.array(mir, dtype=int)
    return rows, mir, np.where(rows != mir, 2.0, 1.0).astype(e.t)


def wtw(e, u):
    return e.W(e.W(u), False, True)


def dense_solve(e, many):
    """[(ux, uy, uz), ...] for the right-hand sides `many` in the engine's dtype: an elimination of the system in the scaled unknown
    v = W uz on the packed rows of the cone,
        [P A' Gs'; A 0 0; Gs 0 -I] [ux; uy; v] = [bx; by; W^-T bz],   Gs = W^-T G,   uz = W^-1 v,
    and two steps of refinement on the residual of K itself, with W'W uz applied as W'(W uz).  The refinement is not an ornament.
    An updated scaling carries r_k and rti_k that are inverse transposes of each other only to eps sqrt(lmbda_max / lmbda_min), 3e-15
    in longdouble and 3e-12 in float64 at mu = 1e-9, so the scaled system alone, which is built from rti_k, answers for a matrix that
    is K only to that; K is the one with W'W from r_k, which the kernel's residual uses too.  (With W'W as an explicit matrix in one
    elimination the residual of a solve is eps |W'W| |uz|, 1e-11 in longdouble, and the identity between the two modes sees it.)"""
    t, n, p, N = e.t, len(e.c), e.p, e.N
    rows, mir, w = packed(e)
    Np = len(rows)
    Gp = e.W(e.G, True, True)[rows]
    K = np.zeros((Np + n + p, Np + n + p), dtype=t)
    K[:Np, :Np] = -np.eye(Np, dtype=t)
    K[:Np, Np:Np + n] = Gp
    K[Np:Np + n, :Np] = (w[:, None] * Gp).T
    K[Np:Np + n, Np:Np + n] = e.P
    K[Np:Np + n, Np + n:] = e.A.T
    K[Np + n:, Np:Np + n] = e.A
    Kinv = eliminate(K, np.eye(len(K), dtype=t))

    def solve(bx, by, bz):
        u = Kinv @ np.concatenate([e.W(bz, True, True)[rows], bx, by])
        v = np.zeros(N, dtype=t)
        v[rows] = u[:Np]
        v[mir] = u[:Np]
        return u[Np:Np + n], u[Np + n:], e.W(v, True)

    out = []
    for rhs in many:
        bx, by, bz = (np.asarray(v, dtype=t) for v in rhs)
        ux, uy, uz = solve(bx, by, bz)
        for _ in range(2):
            dx, dy, dz = solve(bx - (e.P @ ux + e.A.T @ uy + e.G.T @ uz), by - e.A @ ux, bz - (e.G @ ux - wtw(e, uz)))
            ux, uy, uz = ux + dx, uy + dy, uz + dz
        out.append((ux, uy, uz))
    return out


def reduced_solve(e, rhs, refinement):
    """(ux, uy, uz) as the kernel computes them: the reduced solve, uz = W^-1 (W uz), and `refinement` times the residual of the
    full system and a solve with the same factors."""
    def solve(bx, by, bz):
        x, y, wz = e.ksolve(bx, by, bz)
        return x, y, e.W(wz, True)
    bx, by, bz = (np.asarray(v, dtype=e.t) for v in rhs)
    ux, uy, uz = solve(bx, by, bz)
    for _ in range(refinement):
        dx, dy, dz = solve(bx - (e.P @ ux + e.A.T @ uy + e.G.T @ uz), by - e.A @ ux, bz - (e.G @ ux - wtw(e, uz)))
        ux, uy, uz = ux + dx, uy + dy, uz + dz
    return ux, uy, uz


def symmetric(e, v, dtype=None):
    """The vector (or the columns of the matrix) v with every 's' block the symmetric matrix of its lower triangle; e: an
    engine or a batch."""
    return SDN.symmetrise(np.array(v, dtype=dtype or getattr(e, "t", None)), e.Ms, e.sd if hasattr(e, "sd") else e.s)


def rhs_vjp(e, gx):
    return -np.asarray(gx, dtype=e.t), np.zeros(e.p, dtype=e.t), np.zeros(e.N, dtype=e.t)


def rhs_jvp(e, d):
    """The right-hand side of forward mode at the engine's point; a missing name is zero; the lower triangles of dP and of the
    's' blocks of dG and dh are read."""
    t, n, p, N = e.t, len(e.c), e.p, e.N
    get = lambda k, shape: np.asarray(d[k], dtype=t) if d.get(k) is not None else np.zeros(shape, dtype=t)      # noqa: E731
    dP = get("P", (n, n))
    dP = np.tril(dP) + np.tril(dP, -1).T
    dG, dh = symmetric(e, get("G", (N, n))), symmetric(e, get("h", N))
    dA, db = (get("A", (p, n)), get("b", p)) if p else (np.zeros((0, n), dtype=t), np.zeros(0, dtype=t))
    x, y, z = e.x.a, e.y.a, e.z.a
    return -(dP @ x + get("q", n) + dG.T @ z + dA.T @ y), db - dA @ x, dh - dG @ x


def inner(e, grads, d):
    """<grads, d> over the six data: dP by its lower triangle mirrored, the 's' blocks of dG and dh likewise, both triangles
    counted -- the inner product under which grads['G'] and grads['h'] are the gradients with respect to symmetric blocks."""
    d = dict(d)
    for k in ("G", "h"):
        if d.get(k) is not None:
            d[k] = symmetric(e, d[k], np.asarray(grads[k]).dtype)
    return inner_plain(grads, d)


# ---- a whole batch
def _solver(method, refinement):
    if method == "reduced":
        return lambda e, many: [reduced_solve(e, rhs, refinement) for rhs in many]
    return dense_solve


def derivatives(M, sol, gx=None, d=None, method="longdouble", refinement=1, centering=0, centol=np.inf, shared=(), which=None,
                trajectories=None):
    """(V, J): coneqp_batch_vjp for the cotangent gx and coneqp_batch_jvp for the perturbations d restated on the batch M at
    `sol`; None for a mode whose input is None.  method: 'longdouble' or 'float64' (engine and dense elimination in that dtype)
    or 'reduced' (float64, as the kernel).  The layout is that of qp_batch_diff_numpy.derivatives with N rows, plus 'centrality'
    and 'centering steps'.  trajectories: {member: trajectory(...)} computed before, for a table over several caps."""
    solve = _solver(method, refinement)
    dt = np.float64 if method == "reduced" else getattr(np, method)
    B, n, N, p = M.B, M.n, M.N, M.p
    z0 = lambda *shape: np.zeros(shape, dt)                                             # noqa: E731
    V = {"ux": z0(n, B), "uy": z0(p, B), "uz": z0(N, B), "exit": np.zeros(B, dtype=np.int64), "P": z0(B, n, n), "q": z0(n, B),
         "G": z0(B, N, n), "h": z0(N, B), "A": z0(B, p, n), "b": z0(p, B), "centrality": np.full(B, np.nan),
         "centering steps": np.zeros(B, dtype=np.int64)}
    J = {"x": z0(n, B), "y": z0(p, B), "z": z0(N, B), "s": z0(N, B), "exit": np.zeros(B, dtype=np.int64),
         "centrality": np.full(B, np.nan), "centering steps": np.zeros(B, dtype=np.int64)}
    for k in (range(B) if which is None else which):
        e, code, cen, steps = None, EXIT_SKIPPED, np.nan, 0
        if sol["exit"][k] == 0:
            traj, tcode = trajectories[k] if trajectories is not None else trajectory(M, k, sol, dt, centering, centol)
            e, code, cen, steps = centred(traj, tcode, centering, centol)
        if code == EXIT_DONE:
            many = ([rhs_vjp(e, gx[:, k])] if gx is not None else []) + ([rhs_jvp(e, QDN.member_perturbation(d, k))] if d is not None else [])
            try:
                res = solve(e, many)
            except ArithmeticError:
                code, cen = EXIT_FAILED, np.nan
        for R in (V, J):
            R["exit"][k], R["centrality"][k], R["centering steps"][k] = code, cen, steps
        if code:
            continue
        if gx is not None:
            ux, uy, uz = res[0]
            V["ux"][:, k], V["uy"][:, k], V["uz"][:, k] = ux, uy, uz
            g = QDN.gradients(e.x.a, e.y.a, e.z.a, ux, uy, uz)
            for name in NAMES:
                if name in "PGA":
                    V[name][k] = g[name]
                else:
                    V[name][:, k] = g[name]
        if d is not None:
            dx, dy, dz = res[-1]
            J["x"][:, k], J["y"][:, k], J["z"][:, k] = dx, dy, dz
            # the kernel takes ds = -W'W dz from the third block row, bz - G dx: W'W dz loses digits on the rows that are not active
            J["s"][:, k] = many[-1][2] - e.G @ dx if method == "reduced" else -wtw(e, dz)
    for name in shared:
        V[name] = V[name].sum(axis=0) if name in "PGA" else V[name].sum(axis=1)
    if not p:
        V["A"] = V["b"] = None
    return (V if gx is not None else None), (J if d is not None else None)


def direction(M, seed, scale=1.0):
    """One random direction in all six data of the batch M, per member; dP and the 's' blocks of dG and dh symmetric."""
    rng = np.random.default_rng(seed)
    B, n, N, p = M.B, M.n, M.N, M.p
    dP = rng.standard_normal((B, n, n))
    dG, dh = rng.standard_normal((B, N, n)), rng.standard_normal((N, B))
    for k in range(B):
        SDN.symmetrise(dG[k], M.Ms, M.s)
    SDN.symmetrise(dh, M.Ms, M.s)
    return {"P": scale * 0.5 * (dP + dP.transpose(0, 2, 1)), "q": scale * np.asfortranarray(rng.standard_normal((n, B))),
            "G": scale * dG, "h": scale * np.asfortranarray(dh), "A": scale * rng.standard_normal((B, p, n)) if p else None,
            "b": scale * np.asfortranarray(rng.standard_normal((p, B))) if p else None}


def moved(M, d, eps):
    """The batch M moved by eps along the direction d."""
    add = lambda a, v: a if v is None or a is None else a + eps * v                     # noqa: E731
    return types.SimpleNamespace(**dict(vars(M), P=add(M.P, d["P"]), q=add(M.q, d["q"]), G=add(M.G, d["G"]), h=add(M.h, d["h"]),
                                        A=add(M.A, d["A"]), b=add(M.b, d["b"])))


def cotangent(M, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((M.n, M.B)))


def vjp_distance(V, ref, k, names=("ux", "uy", "uz", "P", "G", "A")):
    """The largest distance in units of the rule over the outputs of member k of reverse mode."""
    worst = 0.0
    for name in names:
        if ref.get(name) is None or V.get(name) is None:
            continue
        a, b = (v[name][k] if name in "PGA" else v[name][:, k] for v in (V, ref))
        if np.size(b):
            worst = max(worst, rule(a, b))
    return worst


def jvp_distance(J, ref, k):
    return max(rule(J[name][:, k], ref[name][:, k]) for name in ("x", "y", "z", "s") if ref[name].shape[0])


# ---- the table of DESIGN section 21
CAPS, REFINEMENTS, THRESHOLDS = (0, 2, 4, 6, 8), (0, 1, 2), (1e-2, 1e-4, 1e-6, 1e-8)
FULL_CAP, FULL_TOL = 16, 1e-13


def _worst(V, J, Vr, Jr, members):
    return max([max(vjp_distance(V, Vr, k), jvp_distance(J, Jr, k)) for k in members] + [0.0])


def table(name, centol, caps=CAPS, refinements=REFINEMENTS, thresholds=THRESHOLDS, which=None):
    """What the defaults of 'centering' and 'centol' are chosen from, on batch(name) at solved(name), both modes with the cotangent
    and the direction of the tests; distances in units of the rule, the worst over the members and over all outputs.
      'rounding'    {(cap, refinement): the float64 restatement ('reduced') with that cap and `centol` against the longdouble
                    restatement that goes on centring within the same cap until FULL_TOL, over the members both end with exit 0:
                    rounding, and what the threshold leaves}
      'exits'       {cap: the exits of the float64 restatement}
      'truncation'  {threshold: (the longdouble restatement stopped at that threshold against the one centred to FULL_TOL,
                    the largest number of steps a member takes to the threshold)}; threshold None: the point as it is
      'skipped'     the members whose solution or scaling fails (exit 1 or 2 at every cap)."""
    M, sol = batch(name), solved(name)
    which = list(range(M.B)) if which is None else list(which)
    gx, d = cotangent(M, 5), direction(M, 6)
    T64 = {k: trajectory(M, k, sol, np.float64, max(caps), centol) for k in which if sol["exit"][k] == 0}
    TLD = {k: trajectory(M, k, sol, np.longdouble, FULL_CAP, FULL_TOL) for k in T64}
    run = lambda method, ref, cap, tol, T: derivatives(M, sol, gx, d, method, ref, cap, tol, which=which, trajectories=T)     # noqa: E731
    out = {"rounding": {}, "exits": {}, "truncation": {}, "skipped": []}
    for cap in caps:
        Vr, Jr = run("longdouble", 0, cap, centol, TLD)
        for ref in refinements:
            V, J = run("reduced", ref, cap, centol, T64)
            both = [k for k in which if V["exit"][k] == 0 and Vr["exit"][k] == 0]
            out["rounding"][cap, ref] = _worst(V, J, Vr, Jr, both)
            out["exits"][cap] = V["exit"][which].tolist()
    full = {k: (t[-1:], c if not t else 0) for k, (t, c) in TLD.items()}
    Vf, Jf = run("longdouble", 0, 0, np.inf, full)
    for tol in (None,) + tuple(thresholds):
        if tol is None:
            cut = {k: ([t[0]], 0) for k, (t, c) in TLD.items() if t}
        else:
            cut = {k: ([next((s for s in t if s[1] <= tol), t[-1])], 0) for k, (t, c) in TLD.items() if t}
        steps = [0 if tol is None else next((i for i, s in enumerate(t) if s[1] <= tol), FULL_CAP + 1) for t, c in TLD.values() if t]
        V, J = run("longdouble", 0, 0, np.inf, {**full, **cut})
        both = [k for k in which if V["exit"][k] == 0 and Vf["exit"][k] == 0]
        out["truncation"][tol] = (_worst(V, J, Vf, Jf, both), max(steps + [0]))
    out["skipped"] = [k for k in which if sol["exit"][k] != 0 or not T64[k][0]]
    return out


# The float64 restatement at the defaults (centering 8, centol 1e-6, refinement 1) against the longdouble one in units of the rule, the
# worst member and output of each batch, as tests/test_coneqp_batch_diff_cpu.py::test_table_of_defaults measured it.
# tests/test_coneqp_batch_diff_gpu.py allows the device the larger of the rule and 10 x this: the rule on every batch but one.
ROUNDING = {"absent-q": 8.06e-3, "absent-qs": 3.47e-6, "absent-s": 1.58e-4, "independence": 8.93e-2, "mixed": 5.29e-4, "p-zero": 1.24e-2,
            shape_name(SHAPES[0]): 4.45e-6, shape_name(SHAPES[1]): 4.50e-4, shape_name(SHAPES[2]): 2.89e-2, shape_name(SHAPES[3]): 1.08e-2,
            shape_name(SHAPES[4]): 1.30e-1, shape_name(SHAPES[5]): 1.93e-2, shape_name(SHAPES[6]): 5.82e-7}
