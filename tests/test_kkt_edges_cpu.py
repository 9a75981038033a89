"""The cases of kkt_edge_cases.py on the host: together they must reach every lane, workgroup and grid edge of the orthant KKT-step
kernels (csrc/kkt.hip) that tests/test_kkt_edges_gpu.py is there for, and the bound (K + R) 2^-52 T must admit the same formulas
evaluated in plain float64 numpy on every case -- before it is asked of the device.  A case that fails the bound check gets another
seed or other data; the rule stays.  No device."""
import numpy as np
import pytest

import kkt_edge_cases as kc
from kkt_edge_cases import F8, LD


def test_coverage():
    cov = kc.coverage()
    missing = []

    def need(key, want):
        have = cov[key]
        if isinstance(want, set):
            if not want <= have:
                missing.append((key, sorted(want - have, key=str)))
        elif have != want:
            missing.append((key, have))

    # elementwise (GS_LOOP, 2048 x 256 threads): both sides of a workgroup, of the cap, and a second trip of every thread
    need("elem_mod256", {0, 1, 255})
    need("elem_over_cap", {False, True})
    assert 524288 in kc.ELEM_SIZES and 524289 in kc.ELEM_SIZES and max(kc.ELEM_SIZES) == 1048577 > 2 * 524288
    # reductions: per = ceil(n / 256) on both sides of 1 and of 256 (a thread's second trip at per = 257)
    need("red_mod256", {0, 1, 63, 64, 255})
    need("red_per", {1, 2, 256, 257})
    need("red_second_trip", {False, True})
    need("plants", {"first", "last", "chunk_end", "chunk_start", "second_trip"})
    need("multi_counts", {1, 7, 32})
    need("multi_mixed", True)
    need("multi_empty_sum", True)
    # CCS products
    need("spmv_t_lens", {0, 1, 15, 16, 17, 31, 32, 33, 100})
    need("spmv_t_n", {1, 16, 17, 32769})
    need("spmv_t_empty_ends", True)
    need("spmv_t_over_cap", {False, True})
    need("spmv_n_rowlens", {0, 1, 300})
    need("spmv_n_over_cap", {False, True})
    need("spmm_over_cap", True)
    need("spmm_lens", {0, 1, 16, 17})
    need("gemv_m_mod256", {0, 1, 255})
    need("gemv_blocks", {1, 2, 3})
    need("gemv_n_mod4", {(False, 0), (False, 1), (False, 2), (False, 3), (True, 0), (True, 1), (True, 3)})
    need("pack_blocks", {1, 2, 3})
    need("pack_mod256", {0, 1, 2, 255})
    # assembly: product lists around the four lanes of an entry, and 4 snz around a workgroup
    need("atda_lens", set(kc.ATDA_LENGTHS))
    if not any(v >= 64 for v in cov["atda_lens"]):
        missing.append(("atda_lens", ">= 64"))
    need("atda_snz", {1, 63, 64, 65})
    need("atda_4snz_mod256", {(0, 4), (0, 252), (1, 0), (1, 4)})
    need("atda_flags", {"dense_row", "empty_row", "empty_col", "ml1", "P", "noP", "Pdiag", "Plower"})
    # fused kernels: longest column and row on both sides of every lane count, every kernel instantiation, the caps
    need("fused_max_col", set(kc.FUSED_LONGEST))
    need("fused_max_row", set(kc.FUSED_LONGEST))
    need("fused_empty", True)
    need("fused_lanes_col", {4, 8, 16})
    need("fused_lanes_row", {4, 8, 16})
    need("fused_residual_kernels", {(8, 4), (8, 16), (16, 4), (16, 16)})
    need("fused_rows_over_cap", True)
    need("fused_cols_over_cap", True)
    need("fused_post_x_over_cap", True)
    need("half_ml", set(kc.HALF_ML))
    need("half_n", set(kc.HALF_N))
    need("half_p", set(kc.HALF_P))
    need("half_host_zz", {False, True})
    need("half_ws3", {False, True})
    need("half_x_over_cap", True)
    assert not missing, missing


def test_launch_rules_restated():
    """lanes_for and groups16 as launch_kkt_pre / launch_kkt_post read them"""
    assert [kc.lanes_for(v) for v in (0, 1, 4, 5, 8, 9, 16, 17, 33)] == [16, 4, 4, 8, 8, 16, 16, 16, 16]
    assert kc.groups16(262144) == 16384 and kc.groups16(262145) == 16384 and (262145 * 16 + 255) // 256 == 16385
    assert kc.groups16(262145, 4) == 4097
    assert [kc.red_per(n) for n in (1, 256, 257, 65536, 65537)] == [1, 1, 2, 256, 257]
    assert kc.red_depth(65536) == 20 and kc.red_depth(65537) == 21


def worst(pairs):
    """largest ratio of float64 against the reference over the outputs; pairs: (float64 Out or dict, reference Out or dict)"""
    w = 0.0
    for got, ref in pairs:
        if isinstance(ref, dict):
            assert set(got) == set(ref)
            for k in ref:
                w = max(w, kc.ratio(got[k].ref, ref[k]))
        else:
            w = max(w, kc.ratio(got.ref, ref))
    return w


def both(f, *a, **kw):
    return f(F8, *a, **kw), f(LD, *a, **kw)


@pytest.mark.parametrize("n", kc.ELEM_SIZES)
def test_bound_admits_float64_elementwise(n):
    v = kc.elem_data(n)
    pairs = [both(kc.e_compute_scaling, v["s"], v["z"]), both(kc.e_update_scaling, v["s"], v["z"], v["d"])]
    for lsq in (v["lsq"], None):
        for ws3 in (v["ws3"], None):
            pairs.append(both(kc.e_newton_rhs, lsq, ws3, v["shift"], v["scale"], v["rz"], v["lm"], v["d"]))
    pairs.append(both(kc.e_step_post, v["dtau"], v["z1"], v["lm"], v["ds"], v["dz"]))
    pairs.append(both(kc.e_lp_update, v["step"], v["dsp"], v["dzp"], v["d"], v["lm"]))
    pairs += [both(kc.e_mul, v["x"], v["y"]), both(kc.e_div, v["x"], v["lm"]), both(kc.e_mul, v["y"], v["y"])]
    pairs += [both(kc.e_axpy, v["a"], v["x"], v["y"]), both(kc.e_lincomb, v["a"], v["x"], v["b"], v["y"]),
              both(kc.e_lincomb, v["a"], v["x"], 0.0, v["y"]), both(kc.e_scal, v["a"], v["x"]), both(kc.e_addc, v["c"], v["x"]),
              both(kc.e_xmy, v["a"], v["x"], v["y"], v["b"], v["zz"]), both(kc.e_xmy, v["a"], v["x"], v["y"], 0.0, v["zz"])]
    w = worst(pairs)
    print("elementwise n=%d: float64 error / bound %.3f" % (n, w))
    assert w <= 1.0


@pytest.mark.parametrize("n", kc.RED_SIZES)
def test_bound_admits_float64_reductions(n):
    x, y = kc.red_data(n)
    w = worst([both(kc.r_dot, x, y)])
    print("dot n=%d: float64 error / bound %.3f" % (n, w))
    assert w <= 1.0
    for name, idx in kc.max_step_plants(n).items():
        assert 0 <= idx < n, (name, idx)


def test_bound_admits_float64_ccs_products():
    w = 0.0
    rng = np.random.default_rng(5)
    for mat in kc.spmv_t_mats() + [kc.spmm_mat()]:
        x, y = kc.spread(rng, mat.m), kc.spread(rng, mat.n)
        for alpha, beta in kc.SPMV_AB:
            w = max(w, worst([both(kc.c_spmv_t, mat, alpha, x, beta, y)]))
    for mat in kc.spmv_n_mats():
        x, y = kc.spread(rng, mat.n), kc.spread(rng, mat.m)
        for beta in (0.0, 1.0, -0.5):
            w = max(w, worst([both(kc.c_spmv_n, mat, 2.0, x, beta, y)]))
    for m in kc.GEMV_M:
        for n in kc.GEMV_N:
            A, x, y = kc.spread(rng, m * n).reshape(m, n), kc.spread(rng, n), kc.spread(rng, m)
            for beta in (0.0, -0.5):
                w = max(w, worst([both(kc.c_dense_gemv, A, x, 1.5, beta, y)]))
    print("CCS products: float64 error / bound %.3f" % w)
    assert w <= 1.0


def test_bound_admits_float64_assembly():
    w = 0.0
    for case in kc.atda_cases():
        for sq in (False, True):
            (g, lens), (r, _) = kc.a_assemble(F8, case, sq), kc.a_assemble(LD, case, sq)
            w = max(w, kc.ratio(g.ref, r))
            # an entry without products is the entry of P, to the bit
            assert np.all(g.ref[lens == 0] == r.ref[lens == 0].astype(F8))
    print("assembly: float64 error / bound %.3f" % w)
    assert w <= 1.0


def test_bound_admits_float64_fused():
    w = 0.0
    rng = np.random.default_rng(9)
    for mat in kc.fused_mats() + kc.fused_big_mats():
        tmat = kc.transpose_ccs(mat.m, mat.n, mat.cp, mat.ri, mat.vx)
        di = kc.spread(rng, mat.m, signed=False)
        xin, zin, x2 = kc.spread(rng, mat.n), kc.spread(rng, mat.m), kc.spread(rng, mat.n)
        w = max(w, worst([both(kc.f_pre, mat, di, -0.75, xin, zin), both(kc.f_post, mat, tmat, di, 0.625, -1.5, zin, x2)]))
        x, z, s, c, h = x2, zin, kc.spread(rng, mat.m), xin, kc.spread(rng, mat.m)
        w = max(w, worst([both(kc.f_residuals, mat, tmat, x, z, s, c, h, 0.8125)]))
    print("fused: float64 error / bound %.3f" % w)
    assert w <= 1.0


@pytest.mark.parametrize("ml,n,p,host_zz,with_ws3", kc.half_cases())
def test_bound_admits_float64_second_half(ml, n, p, host_zz, with_ws3):
    v = kc.half_data(ml, n, p)
    zz = 2.75 if host_zz else None
    (g, gz), (r, rz) = kc.h_dtau(F8, v, ml, n, p, zz), kc.h_dtau(LD, v, ml, n, p, zz)
    w = kc.ratio(g.ref, r)
    if rz is not None:
        w = max(w, kc.ratio(gz.ref, rz))
    dtau = float(g.ref[0])
    w = max(w, worst([both(kc.e_step_post, dtau, v["z1"], v["lm"], v["ds"], v["dz"], with_ws3), both(kc.e_axpy, dtau, v["x1"], v["dx"])]))
    print("second half ml=%d n=%d p=%d: float64 error / bound %.3f" % (ml, n, p, w))
    assert w <= 1.0
