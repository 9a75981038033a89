"""The orthant KKT-step kernels of csrc/kkt.hip at their lane, workgroup and grid edges, through the `_dev` entries of the C ABI
(the way test_kkt_gpu.py::test_fused_iteration_entries_against_numpy reaches them), each against a numpy.longdouble restatement
of the formula in its comment, entry by entry, to the derived bound |got - ref| <= (K + R) 2^-52 T of kkt_edge_cases.py (which
test_kkt_edges_cpu.py checks on the host first); copies and maxima to the bit.  kkt_edge_child.py holds the device side; the
sentinels behind every buffer and in the padding rows of every strided output are checked there.

Sections: 1 elementwise kernels at both sides of a workgroup and of the 2048-workgroup cap; 2 the fixed-tree reductions at both
sides of a chunk, of a thread's second trip, with the extreme element planted at every edge of a chunk, and reduce_multi against the
single calls; 3 the CCS products at column lengths around the 16 lanes and past the caps, the dense helpers; 4 the assembly
S = G' diag(w) G (+ P) with product lists around its four lanes, its bit equalities, and the contract of the header for P (the
lower triangle is read, repeated positions are summed as stored, every slot is written once); 5 the fused kernels of an
interior-point iteration with the longest row and column at both sides of 4, 8 and 16 lanes, hinted against 16 lanes bit for
bit, two right-hand sides against one, past the caps, and the second half of f6_no_ir; 6 the same cases under KVX_LP_UNFUSED=1
and the assembly under KVX_ATDA_LPE=1 and 2 in children, one at a time.

Largest error / bound per section on an MI355X (every test prints its own; nothing is asserted of them but <= 1):
    1 elementwise 0.500 (one rounding against 2^-52: addc, lincomb with b = 0, ssqr)      2 reductions 0.020, reduce_multi 0.026
    3 spmv 'T' 0.185, 'N' 0.204, spmm_t 0.240, dense_gemv 0.427                              4 assembly 0.307, one and two lanes 0.307,
    repeated positions of P 0.227      5 pre / post / residuals 0.500 (xout, one rounding), update_x 0.250, second half 0.328
The file takes about 10 s."""
import json
import os
import subprocess
import sys
import time

import pytest

import kkt_edge_cases as kc
import kkt_edge_child as dev
from kvxopt_amd import _lib

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kkt_edge_child.py")
CHILD_TIMEOUT = 300
DEAD = {"stop": None}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


@pytest.fixture(autouse=True)
def _sentinels():
    """the 64 doubles behind every buffer a test made are what they were"""
    dev.Buf.live = []
    yield
    dev.Buf.check_all()


def report(what, R):
    print("%s: largest error / bound %.3f (%s)" % (what, R.worst(), max(R, key=R.get) if R else "-"))
    assert R.worst() <= 1.0


# ---- 1 ----
@pytest.mark.parametrize("n", kc.ELEM_SIZES)
def test_elementwise(n):
    """every elementwise entry at n: NT scaling, the Newton right-hand side in its four forms, step_post with and without ws3, the
    update, scale with 1 and 3 columns and ldx > n, scale2 both ways, sprod / sinv / ssqr, axpy / lincomb (b = 0 with NaN in y, z
    aliasing x, z aliasing y) / scal / addc / fill / xmy (b = 0 with NaN in z) / copy_strided.  R per entry: kkt_edge_cases.e_*."""
    report("elementwise n=%d" % n, dev.run_elementwise(n))


# ---- 2 ----
@pytest.mark.parametrize("n", kc.RED_SIZES)
def test_reductions(n):
    """sdot to the tree's bound (K = red_depth(n), R = 1); max_step to the bit, with the extreme element at index 0, n - 1, the last
    index of a chunk, the first of the next and b0 + 256; max_step of a positive vector is negative"""
    R, _ = dev.run_reductions(n)
    report("reductions n=%d" % n, R)


def test_reduce_multi():
    """counts 1, 7, 32, mixed kinds, a different n per slot, one empty sum (0.0): every value bit for bit the single call's;
    33 slots: KVX_EINVAL; none: KVX_OK"""
    R, _ = dev.run_multi()
    report("reduce_multi", R)


# ---- 3 ----
@pytest.mark.parametrize("mat", kc.spmv_t_mats(), ids=lambda m: m.name)
def test_spmv_t(mat):
    """K = entries of the column, R = 4 (2 with beta = 0, NaN in y)"""
    report("spmv 'T' %s" % mat.name, dev.run_spmv_t(mat))


@pytest.mark.parametrize("mat", kc.spmv_n_mats(), ids=lambda m: m.name)
def test_spmv_n(mat):
    """the atomic form: K = entries of the row (the order is free), R = 3 (2 with beta = 0, NaN in y); no repeatability asserted"""
    report("spmv 'N' %s" % mat.name, dev.run_spmv_n(mat))


def test_spmm_t():
    report("spmm_t", dev.run_spmm_t(kc.spmm_mat()))


@pytest.mark.parametrize("m", kc.GEMV_M)
def test_dense_gemv(m):
    """n = 0 .. 9 around the four partial sums, 1 and 3 right-hand sides, lda > m, ldx > n, ldy > m, beta = 0 with NaN in y and
    beta != 0: K = n, R = 2 (1 with beta = 0)"""
    report("dense_gemv m=%d" % m, dev.run_dense_gemv(m))


@pytest.mark.parametrize("p", kc.PACK_P)
def test_dense_from_ccs_and_pack_lower(p):
    dev.run_dense_and_pack(p)


# ---- 4 ----
ATDA = kc.atda_cases()


@pytest.mark.parametrize("case", ATDA, ids=lambda c: c.name)
def test_assembly(case):
    """to the bound (K = products + entries of P, R = 2, 3 with the square inside); an entry that only P brings to the bit;
    assemble_sq_dev(di) = ssqr + assemble_dev, the host entry = the device entry, two assemblies: the same bits"""
    R, _ = dev.run_assembly(case)
    report("assembly %s" % case.name, R)


@pytest.mark.parametrize("name", ["pairs_Plower", "dense_row_Plower"])
def test_assembly_reads_the_lower_triangle_of_P(name):
    """include/kvxhip.h: the lower triangle of P is read.  P as a full symmetric matrix and P with an entry above the diagonal give
    the bits of the lower triangle; a position stored twice is summed in the order stored (to the bound, the same bits twice)."""
    case = [c for c in ATDA if c.name == name][0]
    report("assembly, P contract, %s" % name, dev.run_assembly_p_contract(case))


# ---- 5 ----
@pytest.mark.parametrize("mat", kc.fused_mats(), ids=lambda m: m.name)
def test_fused_lanes(mat):
    """pre (K = column entries, R = 4), post (xout R = 1; zout K = row entries, R = 4), residuals (hrx R = 0, rx R = 1, hrz R = 1,
    rz R = 2) with the true max_col_nnz / max_row_nnz and with 0: both to the bound and bit-equal; nrhs = 2 with ldx2 > n bit-equal
    to two calls with nrhs = 1"""
    R, _ = dev.run_fused(mat)
    report("fused %s" % mat.name, R)


@pytest.mark.parametrize("mat", kc.fused_big_mats(), ids=lambda m: m.name)
def test_fused_past_the_caps(mat):
    R, _ = dev.run_fused_big(mat)
    report("fused %s" % mat.name, R)


@pytest.mark.parametrize("ml,n", dev.UPDATE_X_SIZES)
def test_update_x(ml, n):
    R, _ = dev.run_update_x(ml, n)
    report("update_x ml=%d n=%d" % (ml, n), R)


@pytest.mark.parametrize("ml,n,p,host_zz,with_ws3", kc.half_cases())
def test_second_half(ml, n, p, host_zz, with_ws3):
    """dtau (K = the deepest tree of the numerator + the tree of z1'z1, R = 8), z1'z1, the two step bounds as exact maxima of what the
    device wrote, dx, dy (R = 2), ds (R = 4), dz (R = 3), ws3 (R = 6) as functions of the dtau returned"""
    R, _ = dev.run_second_half(ml, n, p, host_zz, with_ws3)
    report("second_half ml=%d n=%d p=%d" % (ml, n, p), R)


# ---- 6 ----
def run_child(mode, env):
    """one child at a time; a child that fails stops the ones after it"""
    if DEAD["stop"]:
        pytest.fail("no further child: " + DEAD["stop"])
    try:
        r = subprocess.run([sys.executable, CHILD, mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        DEAD["stop"] = "the child (%s, %s) ran into its time limit" % (mode, env)
        pytest.fail(DEAD["stop"])
    if r.returncode != 0:
        DEAD["stop"] = "the child (%s, %s) ended with status %d" % (mode, env, r.returncode)
        pytest.fail(DEAD["stop"] + "\n" + r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_fused_against_unfused_at_the_edges():
    """sections 2 and 5 on the same seeds: the outputs' bytes in this process (the fused schedule: one launch per reduction, the
    second stage on the host; the second half of f6_no_ir in two launches) and in a child under KVX_LP_UNFUSED=1 (k_reduce2 on the
    device; sixteen launches) are the same"""
    assert os.environ.get("KVX_LP_UNFUSED", "0") in ("", "0"), "this process must run the fused schedule"
    t0 = time.time()
    here = dev.digest()
    there = run_child("digest", {"KVX_LP_UNFUSED": "1"})
    print("digest of %d cases, %.1f s" % (len(here), time.time() - t0))
    assert sorted(here) == sorted(there)
    assert here == there, [k for k in here if here[k] != there[k]]


@pytest.mark.parametrize("lpe", ["1", "2"])
def test_assembly_with_one_and_two_lanes(lpe):
    """the assembly cases with one and two lanes per entry: another order of summation, the same bound"""
    res = run_child("atda", {"KVX_ATDA_LPE": lpe})
    print("assembly with KVX_ATDA_LPE=%s: largest error / bound %.3f" % (lpe, res["ratio"]))
    assert res["lpe"] == lpe and res["ratio"] <= 1.0
