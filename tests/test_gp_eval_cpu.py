"""Host-side checks of what tests/test_gp_eval_gpu.py rests on (tests/gp_eval_numpy.py): the float64 restatement against the
reference's recorded values (G23) and against numpy.longdouble on every edge case, the plan's two patterns on the edge cases, and
that every case has the segment lengths, column counts and launch sizes that its name promises.  No GPU."""
import os

import numpy as np
import pytest

from kvxopt_amd import cvx

import gp_eval_numpy as R

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G23 = np.load(os.path.join(_GOLD, "g23_gp_eval.npz"))
G23_CASES = [str(c) for c in G23["cases"]]
OUTPUTS = ("f", "Df", "H")


def _plan(cs):
    n, Fp, Fi, Fx = R.as_ccs(cs["F"], cs["sparse"])
    return cvx.GPEval(cs["K"], n, Fp, Fi, Fx, cs["g"]), n, Fp, Fi


def _columns_met(ev, m):
    """Per block the number of columns it meets, from the plan's pattern of Df."""
    return np.bincount(ev.Dfi, minlength=m)


@pytest.mark.parametrize("name", G23_CASES)
def test_restatement_agrees_with_the_reference(name):
    """The rule of test_gp_eval_against_reference with the float64 restatement in the GPU's place: 1e-13 x the sum of absolute
    contributions, and where an output misses that (spread700), the two are within 4 x of each other against longdouble."""
    args = (G23[name + "__K"], G23[name + "__F"], G23[name + "__g"], G23[name + "__x"], G23[name + "__z"])
    r64, rld = R.numpy_eval(*args, np.float64), R.numpy_eval(*args, np.longdouble)
    for k, what in enumerate(OUTPUTS):
        ref, sc = G23[name + "__" + what], r64[3 + k]
        err = np.abs(r64[k] - ref)
        print("G23 %s %s: restatement against the reference, max |err| / scale = %.3e" % (name, what, (err / np.maximum(sc, 1e-300)).max()))
        if np.all(err <= 1e-13 * sc):
            continue
        own, refs = float(np.abs(r64[k] - rld[k]).max()), float(np.abs(ref - rld[k]).max())
        print("   against longdouble: restatement %.3e, reference %.3e" % (own, refs))
        assert own <= 4.0 * refs and refs <= 4.0 * own, (name, what, own, refs)


@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_restatement_alone_stays_inside_the_bound(name):
    """float64 against longdouble is at most 1e-14 x scale on f, Df and H: a tenth of the bound the GPU test applies."""
    _, r64, rld = R.restated(name)
    for k, what in enumerate(OUTPUTS):
        ratio = np.abs(r64[k] - rld[k]) / np.maximum(r64[3 + k], 1e-300)
        print("%s %s: float64 against longdouble, max |err| / scale = %.3e" % (name, what, ratio.max()))
        assert np.all(np.abs(r64[k] - rld[k]) <= 1e-14 * r64[3 + k]), (name, what, float(ratio.max()))


@pytest.mark.parametrize("name", R.NON_CAP_CASES)
def test_plan_patterns_on_the_edge_cases(name):
    cs = R.build(name)
    ev, n, Fp, Fi = _plan(cs)
    R.assert_plan_patterns(ev, cs["K"], n, Fp, Fi)
    # the pattern of Df against the stored entries counted block by block
    seg = R.segment_lengths(cs["K"], cs["F"]) if cs["sparse"] else np.repeat(cs["K"][:, None], n, axis=1)
    assert np.array_equal(_columns_met(ev, cs["K"].size), (seg > 0).sum(axis=1))


def test_cases_sit_where_their_names_say():
    """Segment lengths and columns met, recomputed from F, and the class and launch arithmetic of every case."""
    SM, WV, SW, CAP = R.GP_SMALL_MAX, R.GP_WAVE_MAX, R.GP_SEG_WAVE, R.GRID_CAP
    built = {name: R.build(name) for name in R.NON_CAP_CASES}
    K = {name: cs["K"].tolist() for name, cs in built.items()}
    met = {name: _columns_met(_plan(cs)[0], cs["K"].size).tolist() for name, cs in built.items()}
    seg = {name: R.segment_lengths(cs["K"], cs["F"]) for name, cs in built.items()}
    # the three classes of the log-sum-exp and the passes inside them
    assert K["lse_small_wave"] == [SM - 1, SM, SM + 1, 1] and met["lse_small_wave"] == 4 * [17]
    assert [k % 4 for k in K["lse_small_wave"][:3]] == [3, 0, 1]                      # the masked MFMA tail with c = 17
    assert K["lse_wave_wg"] == [WV - 1, WV, WV + 1, 2] and met["lse_wave_wg"] == 4 * [33]
    assert K["lse_wg_passes"] == [2 * 256 - 1, 2 * 256, 2 * 256 + 1] and met["lse_wg_passes"] == 3 * [16]
    assert K["wave_passes"] == [2 * 64 - 1, 2 * 64, 2 * 64 + 1, 2 * 64 + 2, 3]
    # wavefront gradients: a partly live last workgroup of four, passes of 4 and 5 over 64 lanes, segments on both sides of 64
    waves = seg["lse_wave_wg"][seg["lse_wave_wg"] > SW]
    assert waves.size % 4 != 0 and set(-(-waves // 64)) == {4, 5}
    s = seg["wave_passes"][:4]
    assert (s <= SW).any() and (s > SW).any() and s.min() > 32
    # Gram tiles: every block meets exactly 15 or 16 of the 20 columns, with K mod 4 = 1, 2, 3
    for name, c in (("gram_c15", 15), ("gram_c16", 16)):
        assert K[name] == [5, 18, 67] and met[name] == 3 * [c] and (seg[name] > 0).sum(axis=1).tolist() == 3 * [c]
    # a partly live last row of 16 groups of 16 lanes, and a partly live last workgroup of four wavefronts
    assert K["partial_groups_k3"] == 17 * [3] and len(K["partial_groups_k3"]) % 16 == 1
    assert K["partial_groups_k20"] == 5 * [20] and SM < 20 <= WV and len(K["partial_groups_k20"]) % 4 == 1
    # empty blocks: a middle one and the last; block 0 meets one column; one column is empty
    assert met["empty_blocks"] == [1, 0, 4, 4, 0] and R.EMPTY_BLOCKS["empty_blocks"] == [1, 4]
    assert not built["empty_blocks"]["F"][:, 5].any() and built["empty_blocks"]["F"][:, :5].any(axis=0).all()
    # sparse segments of 64 and 65 entries on every third row
    F = built["sparse_segments"]["F"]
    assert seg["sparse_segments"][0].tolist() == [SW, SW + 1, 1, 200] and seg["sparse_segments"][1, 2:].tolist() == [1, 70]
    assert set(np.diff(np.flatnonzero(F[:200, 0]))) == {3} and set(np.diff(np.flatnonzero(F[:200, 1]))) == {3}
    # exp over- and underflows without the shift, in the wavefront and the workgroup class
    cs = built["spread_wave"]
    u = cs["F"] @ cs["x"] + cs["g"]
    assert K["spread_wave"] == [SM + 1, WV + 1]
    for lo, hi in ((0, 17), (17, 274)):
        assert u[lo:hi].max() > 690 and u[lo:hi].min() < -690 and np.abs(u[lo:hi]).min() < 5
    # the caps: more work items than one trip of the capped grid takes
    cap = {name: R.EDGE_CASES[name] for name in R.CAP_CASES}
    m = {name: len(cs["K"]) for name, cs in cap.items()}
    k = {name: cs["K"][0] for name, cs in cap.items()}
    assert k["cap_group"] <= SM and m["cap_group"] > 16 * CAP
    assert SM < k["cap_wave"] <= WV and m["cap_wave"] > 4 * CAP
    assert k["cap_wg_fsc"] > WV and m["cap_wg_fsc"] > CAP and m["cap_wg_fsc"] * k["cap_wg_fsc"] == 1053700 > 256 * CAP
    assert k["cap_grad_wave"] > SW and m["cap_grad_wave"] * cap["cap_grad_wave"]["n"] > 4 * CAP
    assert k["cap_grad_thread"] <= SW and m["cap_grad_thread"] * cap["cap_grad_thread"]["n"] > 256 * CAP
    assert all(len(set(cs["K"])) == 1 and cs["density"] == 1.0 for cs in cap.values())


def test_empty_blocks_in_the_restatement():
    """f_i = logsumexp(g_i), an empty row of Df and no contribution to H, whatever z_i is."""
    cs, r64, _ = R.restated("empty_blocks")
    off = R.block_offsets(cs["K"])
    z = cs["z"].copy()
    for b in R.EMPTY_BLOCKS["empty_blocks"]:
        gb = cs["g"][off[b]:off[b + 1]]
        assert abs(r64[0][b] - (gb.max() + np.log(np.exp(gb - gb.max()).sum()))) <= 1e-15
        assert not r64[1][b].any()
        z[b] = 123.0
    assert np.array_equal(R.numpy_eval(cs["K"], cs["F"], cs["g"], cs["x"], z, np.float64)[2], r64[2])


@pytest.mark.parametrize("name", ["partial_groups_k3", "partial_groups_k20"])
def test_stacked_and_per_block_restatement_are_equal(name):
    """The same bytes in float64; in longdouble the same values (its padding bytes are not defined)."""
    cs = R.build(name)
    args = (cs["K"], cs["F"], cs["g"], cs["x"], cs["z"])
    for a, b in zip(R.numpy_eval(*args, np.float64), R.numpy_eval_equal_k(*args, np.float64)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    for a, b in zip(R.numpy_eval(*args, np.longdouble), R.numpy_eval_equal_k(*args, np.longdouble)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
