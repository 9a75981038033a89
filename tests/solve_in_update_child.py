"""Child process of test_solve_in_update_gpu.py: KVX_SOLVE_IN_UPDATE_TILES is read once per factor, so each setting of it runs
in a process of its own.  For every case named on the command line the child factors three times (eagerly, under capture, from
the replayed graph), solves, and writes the bits -- the factor's values, diag(), x, or the failing column of a case that is not
positive definite -- and the launch counters to <out dir>/<case>.npz.

Also imported by the test for the cases.  A case is a forest of fronts known in advance (chol_class_cases.py: natural order, no
amalgamation), the smallest shapes at which the fused chain step (k_syrk_solve) can go wrong."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import chol_class_cases as cc

KNOB = "KVX_SOLVE_IN_UPDATE_TILES"
FORCE = 10**9            # every eligible launch takes the fused step (pairs start at 3000 tiles: none of the cases has a launch that large)

# name -> (designs, (m, k) of the front the case is about)
CASES = {
    # trailing matrix = one partial tile, one row below the panel
    "k128_m129": ([cc.leaf(129, 128)], (129, 128)),
    # last panel 2 columns wide: nbk < 64 in X and in the inverse
    "k130_m200": ([cc.leaf(200, 130)], (200, 130)),
    # no update matrix: the root's shape
    "k192_root": ([cc.root(192)], (192, 192)),
    # row blocks straddle the boundary between the panel and the update matrix; the last block has one row
    "k65_m194": ([cc.leaf(194, 65)], (194, 65)),
    # two fronts of different orders in one launch: two size classes (3 and 9 tile rows at the first step)
    "two_fronts": ([cc.leaf(600, 140), cc.leaf(200, 130)], (600, 140)),
}
# not positive definite: the failing column lies in the second diagonal block of the root, factored by the fused step of panel 0
NOTPD = {"notpd_col100": ([cc.root(192)], 100)}
ALL = list(CASES) + list(NOTPD)


def system(name):
    """n, colptr, rowind, values, the case object"""
    designs = CASES[name][0] if name in CASES else NOTPD[name][0]
    case = cc.Case(name, designs)
    n, cp, ri, vx = case.system()
    if name in NOTPD:
        vx = vx.copy()
        vx[cp[NOTPD[name][1]]] = -1.0                      # the diagonal entry of that column
    return n, cp, ri, vx, case


def run(name, out_dir):
    from kvxopt_amd._lib import lib
    from kvxopt_amd.chol import Factor
    n, cp, ri, vx, case = system(name)
    F = Factor(n, cp, ri, "L", opts=cc.OPTS)
    fronts, _, _, _ = cc.realised(F)
    assert sorted(fronts) == case.fronts, (name, sorted(fronts), case.fronts)
    lib().kvx_dbg_syrk_solve_count(1)
    out = {}
    if name in NOTPD:
        minors = []
        for rep in range(3):                               # eager, capture, replay
            try:
                F.factorize(vx)
                minors.append(-1)
            except ArithmeticError as e:
                minors.append(int(e.args[0]))
        out["minor"] = np.array(minors, dtype=np.int64)
    else:
        B = np.random.default_rng(n).standard_normal((n, 2))
        for rep in range(3):
            F.factorize(vx)
            _, _, Lx = F.get_factor()
            X = np.asfortranarray(B.copy())
            F.solve(X)
            out["Lx%d" % rep], out["diag%d" % rep], out["x%d" % rep] = Lx.copy(), F.diag().copy(), X
    out["perm"] = np.asarray(F.perm())
    out["fused_launches"] = np.array([int(lib().kvx_dbg_syrk_solve_count(0))], dtype=np.int64)
    np.savez(os.path.join(out_dir, name + ".npz"), **out)


def main():
    from kvxopt_amd import _lib
    _lib.require_device()
    out_dir = sys.argv[1]
    for name in sys.argv[2:]:
        run(name, out_dir)
        print("done", name, flush=True)
    print("RESULT ok", flush=True)


if __name__ == "__main__":
    main()
