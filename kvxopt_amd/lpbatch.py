"""Many small dense linear programs in one launch, with infeasibility certificates:

    lp_batch(c, G, h, A=None, b=None, options=None) -> dict          also kvxopt_amd.solvers.lp_batch

solves  minimize c_b'x  s.t.  G_b x + s = h_b, s >= 0,  A_b x = b_b  for b = 0..B-1 by the algorithm of solvers.lp (conelp's
self-dual embedding, coneprog.py:662-1436 on the orthant, the Newton systems of misc.kkt_chol2), one workgroup per member from
its starting point to its status or its certificate (csrc/lp_batch.hip, kvx_lp_batch_solve).  It is the companion of
solvers.qp_batch for what coneqp cannot say: an infeasible or unbounded member comes back "primal infeasible" or "dual
infeasible" with its scaled certificate, not "unknown" after maxiters iterations -- LP relaxations of sibling branch-and-bound
nodes, feasibility checks of MPC horizons, scenario sweeps, Chebyshev and L1 fits over many windows.

  c        n x B, member b in column b; defines n and B
  h, b     ml x B and p x B, or one column shared by all members
  G, A     each one matrix shared by all members (base.matrix, base.spmatrix or a 2-D array; sparse input is made dense on the
           host) or a float64 array (B, rows, n) with member b in [b]
  limits   1 <= n <= 64, 1 <= ml <= 512, 0 <= p <= n as for qp_batch, and conelp's p + ml >= n: a ValueError outside them --
           solvers.lp is the path for larger problems.  There is no fallback loop.
  options  maxiters, abstol, reltol, feastol as solvers.lp checks them; refinement must be 0 (the orthant's default);
           show_progress is accepted and nothing is printed.  The module-level solvers.options is not read.
           No primalstart / dualstart, no kktsolver, no solver=.

Member b's result is what _ipm.conelp_start plus _ipm.conelp_loop give on that member alone with the dense kkt_chol2 solve: the
starting point with W = I, both pushes into the cone and the optimal-at-iteration-0 return; tau, kappa, dg and lmbda_g; the
constant system (-c, b, h) solved at every iteration; predictor and corrector with sigma = (1 - step)^3, the step rule and the
scaling update of misc.py:444-464; the order of the three tests (optimal or maxiters, then the primal, then the dual
certificate) and the final scalings by 1/tau, 1/(-h'z - b'y) or 1/(-c'x).  kkt_chol2's F['singular'] branch is carried: if the
Cholesky factor of S = G'G at the first factorisation (the one with W = I) fails and p > 0, S := S + A'A for this and every
later factorisation of that member and every solve adds A'by to bx (misc.py:1433-1458, 1526-1527) -- so an LP whose free
variables are held by the equality constraints alone is solved.  Fixed summation order, no atomics; a member's bytes do not
depend on B, on its place or on the other members.

The result has 'status' (B strings: "optimal", "primal infeasible", "dual infeasible" or "unknown"), 'x' (n x B), 'y' (p x B),
's', 'z' (ml x B), float arrays of length B 'gap', 'relative gap', 'primal objective', 'dual objective', 'primal infeasibility',
'dual infeasibility', 'primal slack', 'dual slack', 'residual as primal infeasibility certificate', 'residual as dual
infeasibility certificate' -- nan where the reference's dictionary holds None, as in the tuples of _ipm.conelp_loop -- and int
arrays 'iterations' and 'exit':
  0 optimal; 1 maxiters reached; 2 singular KKT matrix after the first iteration (the iterates scaled by 1/tau);
  3 the factorisation with W = I or the first one failed even after the A'A repair (solvers.lp raises ValueError("Rank(A) < p
    or Rank([G; A]) < n")): that member has zeros in x, y, s, z, 0 iterations and nan statistics, and does not disturb the others;
  4 primal infeasible: y, z are the certificate with h'z + b'y = -1, the member's columns of x and s are nan;
  5 dual infeasible: x, s are the certificate with c'x = -1, the member's columns of y and z are nan."""
from . import _batch
from ._batch import (EXIT_DUAL_INFEASIBLE, EXIT_MAXITERS, EXIT_OPTIMAL, EXIT_PRIMAL_INFEASIBLE, EXIT_RANK,  # noqa: F401
                     EXIT_SINGULAR, MAX_ML, MAX_N, STATUS)
from ._batch import LP_STATS as _STATS

_limit = _batch.limiter("lp_batch", "lp")


def _prepare(c, G, h, A, b, options):
    """Every argument check, on the host; returns what kvx_lp_batch_solve takes."""
    opt = _batch.options("lp_batch", "lp", options, qp=False)
    c, n, B = _batch.members(c, "c")
    _limit("n", n, 1, MAX_N)
    Gv, sG, ml = _batch.matrix(G, "G", n, B, defines="c")
    _limit("ml", ml, 1, MAX_ML)
    hv, sh = _batch.shared_or_batch(h, "h", ml, B, "'h' must be a 'd' matrix of size (%d,1)" % ml)
    p, eqA, eqb = _batch.equalities(A, b, n, B, "c", _limit)
    if p + ml < n:
        raise ValueError("lp_batch: p + ml = %d is outside its limit p + ml >= n = %d (conelp's Rank([G; A]) < n); solvers.lp "
                         "raises the same for one problem" % (p + ml, n))
    return opt, (B, n, ml, p), (_batch.flat(c, B), (Gv, sG), (hv, sh), eqA, eqb)


def lp_batch(c, G, h, A=None, b=None, options=None):
    opt, (B, n, ml, p), data = _prepare(c, G, h, A, b, options)
    return _batch.solve("kvx_lp_batch_solve", [B, n, ml, p], data, opt, B, n, p, ml, _STATS, STATUS)
