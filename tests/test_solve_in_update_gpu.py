"""The chain step whose trailing update solves its own panel rows (k_syrk_solve, KVX_SOLVE_IN_UPDATE_TILES) against the two-launch
step, to the bit: factor values, diag(), x, and the failing column of a matrix that is not positive definite.  The knob is read
once per factor, so each setting runs in a child process (solve_in_update_child.py); two children in all.

The fused step forms X = A Linv' with the products of k_trsm_blk in its order and hands the tile update the operands
k_syrk_trailing<64> would have loaded back, so nothing may differ -- also not between the eager, the captured and the replayed
factorisation of one process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kvxopt_amd import _lib

import solve_in_update_child as child

pytestmark = pytest.mark.gpu


def run_child(knob, out_dir):
    env = {k: v for k, v in os.environ.items() if k != child.KNOB}
    env[child.KNOB] = str(knob)
    os.makedirs(out_dir)
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), out_dir] + child.ALL, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (knob, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    return {name: np.load(os.path.join(out_dir, name + ".npz")) for name in child.ALL}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    _lib.require_device()
    base = tmp_path_factory.mktemp("solve_in_update")
    return run_child(0, str(base / "two_launches")), run_child(child.FORCE, str(base / "fused"))


@pytest.mark.parametrize("name", list(child.CASES))
def test_fused_step_gives_the_bits_of_the_two_launch_step(runs, name):
    two, fused = runs
    assert int(two[name]["fused_launches"][0]) == 0
    assert int(fused[name]["fused_launches"][0]) > 0, "the forced setting did not launch k_syrk_solve"
    assert np.array_equal(two[name]["perm"], fused[name]["perm"])
    for rep in range(3):                                   # eager, capture, replay
        for key in ("Lx", "diag", "x"):
            a, b = two[name]["%s%d" % (key, rep)], fused[name]["%s%d" % (key, rep)]
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (name, key, rep, int((a != b).sum()))
            assert np.all(np.isfinite(b)), (name, key, rep)
    # and the factor is a factor: residual of the solve
    n, cp, ri, vx, _ = child.system(name)
    from kvxopt_amd import workloads
    B = np.random.default_rng(n).standard_normal((n, 2))
    res = np.linalg.norm(workloads.sym_matvec(n, cp, ri, vx, fused[name]["x0"]) - B) / np.linalg.norm(B)
    assert res < 1e-10, (name, res)


@pytest.mark.parametrize("name", list(child.NOTPD))
def test_failing_column_in_a_block_factored_by_the_fused_step(runs, name):
    two, fused = runs
    assert int(fused[name]["fused_launches"][0]) > 0
    want = int(np.flatnonzero(fused[name]["perm"] == child.NOTPD[name][1])[0])      # minor counts the permuted columns
    assert 64 <= want < 128                                # second diagonal block: factored by the update of panel 0
    assert two[name]["minor"].tolist() == [want] * 3, two[name]["minor"]
    assert fused[name]["minor"].tolist() == [want] * 3, fused[name]["minor"]
