"""kvx_gp_eval_dev on the edges of its size classes: the cases of tests/gp_eval_numpy.py (16-lane group | wavefront | workgroup
log-sum-exp at K = 16 | 17 and 256 | 257, thread | wavefront gradients at segments of 64 | 65, Gram tiles at c = 15 | 16 | 17 and
32 | 33 with every K mod 4, partly live groups and wavefronts, blocks that meet no column, the second trip of the grid-stride
loops) against the numpy.longdouble restatement, through cvx.GPEval.eval_ptr."""
import time

import numpy as np
import pytest

from kvxopt_amd import cvx
from kvxopt_amd.devvec import DVec

import gp_eval_numpy as R

pytestmark = pytest.mark.gpu

POISON = -7.25e300
OUTPUTS = ("f", "Df", "H")


def _plan(K, F, g, sparse):
    n, Fp, Fi, Fx = R.as_ccs(F, sparse)
    return cvx.GPEval(K, n, Fp, Fi, Fx, g)


def _evaluate(ev, x, z):
    """The raw buffers f, Dfx, Hx of one kvx_gp_eval_dev call; all three are poisoned before it."""
    n, m = ev.n, ev.nrows
    xd, f = DVec(n, x), DVec(m).fill(POISON)
    Dfx, Hx = DVec(max(ev.Dfi.size, 1)).fill(POISON), DVec(max(ev.Hi.size, 1)).fill(POISON)
    zd = None if z is None else DVec(m, z)
    ev.eval_ptr(xd.ptr, None if z is None else zd.ptr, f.ptr, Dfx.ptr, None if z is None else Hx.ptr)
    return f.get(), Dfx.get(), Hx.get()


def _dense(ev, raw_df, raw_h):
    Df, H = np.zeros((ev.nrows, ev.n)), np.zeros((ev.n, ev.n))
    Df[ev.df_pattern] = raw_df[:ev.Dfi.size]
    H[ev.h_pattern] = raw_h[:ev.Hi.size]
    return Df, H


def _alone(cs, b):
    """Block b of a case as a plan of its own: f and the dense row of Df."""
    off = R.block_offsets(cs["K"])
    rows = slice(off[b], off[b + 1])
    ev = _plan(cs["K"][b:b + 1], cs["F"][rows], cs["g"][rows], cs["sparse"])
    f, raw_df, raw_h = _evaluate(ev, cs["x"], cs["z"][b:b + 1])
    return f, _dense(ev, raw_df, raw_h)[0]


@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_gp_eval_at_the_class_edges(name):
    """|got - longdouble| <= 1e-13 x (sum of absolute contributions) entrywise on f, Df and H, the project's bound for assembled
    values.  Where an output misses it the bound is not loosened: the GPU's worst error against longdouble may be at most 4 x
    that of the float64 restatement (summation order, exp rounding), as in test_gp_eval_against_reference."""
    t0 = time.perf_counter()
    cs, r64, rld = R.restated(name)
    K, x, z = cs["K"], cs["x"], cs["z"]
    m, off = K.size, R.block_offsets(K)
    t1 = time.perf_counter()
    ev = _plan(K, cs["F"], cs["g"], cs["sparse"])
    t2 = time.perf_counter()
    f, raw_df, raw_h = _evaluate(ev, x, z)
    t3 = time.perf_counter()
    # every entry of f and of the value buffers of Df and H was written
    assert not np.any(f == POISON) and not np.any(raw_df[:ev.Dfi.size] == POISON) and not np.any(raw_h[:ev.Hi.size] == POISON)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(raw_df[:ev.Dfi.size])) and np.all(np.isfinite(raw_h[:ev.Hi.size]))
    Df, H = _dense(ev, raw_df, raw_h)
    for k, (what, got) in enumerate(zip(OUTPUTS, (f, Df, H))):
        true, sc = rld[k], r64[3 + k]
        err = np.asarray(np.abs(got - true), dtype=float)
        own = np.asarray(np.abs(r64[k] - true), dtype=float)
        print("%s %s: max |err| / scale = %.3e on the GPU, %.3e in the float64 restatement" % (
            name, what, (err / np.maximum(sc, 1e-300)).max(), (own / np.maximum(sc, 1e-300)).max()))
        if np.all(err <= 1e-13 * sc):
            continue
        gpu_err, ref_err = float(err.max()), float(own.max())
        print("   against longdouble: GPU %.3e, restatement %.3e, ratio %.2f" % (gpu_err, ref_err, gpu_err / ref_err if ref_err else np.inf))
        assert gpu_err <= 4.0 * ref_err, (name, what, gpu_err, ref_err)
    # the line-search form: the same f and Df, the poisoned H buffer untouched
    f2, raw_df2, raw_h2 = _evaluate(ev, x, None)
    assert f2.tobytes() == f.tobytes() and raw_df2.tobytes() == raw_df.tobytes()
    assert np.all(raw_h2 == POISON)
    # a second full call: the same bytes on all three buffers
    f3, raw_df3, raw_h3 = _evaluate(ev, x, z)
    assert f3.tobytes() == f.tobytes() and raw_df3.tobytes() == raw_df.tobytes() and raw_h3.tobytes() == raw_h.tobytes()
    # blocks that meet no column: f_i = logsumexp(g_i), and z_i reaches nothing
    empty = R.EMPTY_BLOCKS.get(name, [])
    for b in empty:
        gb = np.asarray(cs["g"][off[b]:off[b + 1]], dtype=np.longdouble)
        lse = gb.max() + np.log(np.exp(gb - gb.max()).sum())
        assert abs(f[b] - lse) <= 1e-13 * r64[3][b] and not Df[b].any()
    if empty:
        z2 = z.copy()
        z2[empty] = [123.0, 0.0][:len(empty)]
        assert _evaluate(ev, x, z2)[2].tobytes() == raw_h.tobytes()
    # one-term blocks: Df_i = F_i exactly
    for b in np.flatnonzero(K == 1):
        assert np.array_equal(Df[b], cs["F"][off[b]])
    # the same block in the same class at another place of its launch: the same bytes of f and Df
    if name in ("lse_small_wave", "lse_wave_wg"):
        for b in range(m):
            fb, Dfb = _alone(cs, b)
            assert fb.tobytes() == f[b:b + 1].tobytes() and Dfb.tobytes() == Df[b:b + 1].tobytes(), (name, b)
    # past the cap of the grid: a second trip must not read the first trip's blocks again
    if name in R.CAP_CASES:
        for b in (0, m - 1):
            assert _alone(cs, b)[0].tobytes() == f[b:b + 1].tobytes(), (name, b)
    t4 = time.perf_counter()
    print("%s: restatement %.2f s, plan %.2f s, first call with upload %.2f s, whole test %.2f s" % (name, t1 - t0, t2 - t1, t3 - t2, t4 - t0))
