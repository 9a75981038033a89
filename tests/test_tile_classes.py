"""The workgroup numbering of the big fronts' trailing-update launches (tile_classes.hpp), on the CPU.

kvx_dbg_tile_cover runs make_tile_classes for one launch and walks every workgroup id through the decode and the tile guard the
kernels run (the same code, __host__ __device__).  Every tile of every front's update region -- computed here independently from
the region's definition -- must be taken by exactly one workgroup: a tile taken twice is C -= X X' applied twice by racing
workgroups (and, for tile (0, 0), two workgroups factoring the next diagonal block), a tile never taken is an update missing."""
import ctypes
import os

import numpy as np
import pytest

from kvxopt_amd import _lib, workloads
from kvxopt_amd.chol import Factor

import syrk_schedule_child as child

INT_MAX = child.INT_MAX
TILE = 64
MAXCLS = 16


def cover(uonly, hm, hk, kb, klen, col_lim):
    """(counts[front, ti, tj], class table) of one launch"""
    hm = np.ascontiguousarray(hm, dtype=np.int32)
    hk = np.ascontiguousarray(hk, dtype=np.int32)
    count = len(hm)
    tmax = max(int(hm.max(initial=0)) // TILE + 2, 1)
    counts = np.zeros(max(count * tmax * tmax, 1), dtype=np.int32)
    info = np.zeros(70, dtype=np.int64)
    i32p = ctypes.POINTER(ctypes.c_int32)
    rc = _lib.lib().kvx_dbg_tile_cover(int(uonly), hm.ctypes.data_as(i32p), hk.ctypes.data_as(i32p), count, kb, klen, col_lim, tmax,
                                       counts.ctypes.data_as(i32p), _lib.pi(info))
    assert rc == 0
    ncls = int(info[0])
    cls = {"ncls": ncls, "workgroups": int(info[1]), "accepted": int(info[2]), "stray": int(info[3]),
           "first": info[4:5 + ncls].tolist(), "T": info[21:21 + ncls].tolist(), "TC": info[37:37 + ncls].tolist(),
           "wg": info[53:54 + ncls].tolist()}
    return counts[:count * tmax * tmax].reshape(count, tmax, tmax), cls


def region(uonly, m, k, kb, klen, col_lim, tmax):
    """the tiles (ti, tj) of a front's update region in a launch, from its definition (k_syrk_lds)"""
    if kb >= k:
        return np.zeros((tmax, tmax), dtype=np.int32)
    nbk = min(klen, k - kb)
    t0 = min(col_lim, k) if uonly else kb + nbk
    cend = m if (uonly or col_lim == INT_MAX) else min(col_lim, k)
    ti, tj = np.meshgrid(np.arange(tmax), np.arange(tmax), indexing="ij")
    return ((tj <= ti) & (t0 + TILE * ti < m) & (t0 + TILE * tj < cend)).astype(np.int32)


def check_cover(uonly, hm, hk, kb, klen, col_lim):
    counts, cls = cover(uonly, hm, hk, kb, klen, col_lim)
    where = "launch uonly=%d kb=%d klen=%d col_lim=%d fronts %s" % (uonly, kb, klen, col_lim, list(zip(hm, hk)))
    assert cls["stray"] == 0, where
    R = np.stack([region(uonly, hm[f], hk[f], kb, klen, col_lim, counts.shape[1]) for f in range(len(hm))])
    if np.array_equal(counts, R):
        assert cls["accepted"] == int(counts.sum()), where
        return counts, cls
    for f in range(len(hm)):
        dup = np.argwhere(counts[f] > 1)
        assert dup.size == 0, "%s: front %d, tiles %s taken more than once" % (where, f, [tuple(t) for t in dup.tolist()])
        missed = np.argwhere(R[f] > counts[f])
        assert missed.size == 0, "%s: front %d, tiles %s never taken" % (where, f, [tuple(t) for t in missed.tolist()])
        extra = np.argwhere(counts[f] > R[f])
        assert extra.size == 0, "%s: front %d, tiles %s outside the region" % (where, f, [tuple(t) for t in extra.tolist()])
    assert cls["accepted"] == int(counts.sum())
    return counts, cls


# ---- the two lists of the overlap, and one case of each transition --------------------------------------------------------------
def test_near_launch_of_a_512_block_rectangular_then_triangular_class():
    hm, hk = [2100, 1500], [812, 1100]
    counts, cls = check_cover(0, hm, hk, 0, 512, 1024)
    assert cls["ncls"] == 2 and cls["T"] == [25, 16] and cls["TC"] == [5, 0]
    # class 0 has 125 tiles; class 1 (XCD-numbered) starts on a multiple of 8: ids 125 - 127 are padding
    assert cls["first"] == [0, 1, 2] and cls["wg"] == [0, 128, 128 + 8 * ((16 * 17 // 2 + 7) // 8)]


def test_pair_launch_where_both_fronts_end_inside_the_panel():
    hm, hk = [1020, 1019], [127, 1]
    counts, cls = check_cover(0, hm, hk, 0, 128, INT_MAX)
    assert cls["ncls"] == 2 and cls["T"] == [14, 16] and cls["TC"] == [0, 0]
    assert cls["wg"][1] == 112                                       # 14 * 15 / 2 = 105 tiles, then padding to 112
    assert counts[1, 0, 0] == 1


def test_pair_launch_at_a_later_panel():
    check_cover(0, [1276, 1275], [383, 257], 256, 128, INT_MAX)


@pytest.mark.parametrize("T0", [13, 14])
def test_small_triangular_class_then_xcd_numbered_class(T0):
    # K range of 256 columns over the whole trailing matrix: front 0 keeps T0 tile rows, front 1 ends inside the K range and
    # keeps 16 (more tile rows behind a smaller order: a new class, numbered from the next multiple of 8)
    m0 = 256 + 64 * T0
    hm, hk = [m0, 962], [m0, 1]
    counts, cls = check_cover(0, hm, hk, 0, 256, INT_MAX)
    assert cls["T"] == [T0, 16] and cls["TC"] == [0, 0] and cls["wg"][1] % 8 == 0 and cls["wg"][1] > T0 * (T0 + 1) // 2
    assert counts[1, 0, 0] == 1


def test_rectangular_class_then_triangular_class_of_16_rows():
    # near launch of a 1024-column block: front 0's region is 31 x 7 tiles (rectangular, 217 workgroups), front 1's a
    # 16-row triangle (XCD-numbered from workgroup 224)
    hm, hk = [3000, 2040], [1450, 2040]
    counts, cls = check_cover(0, hm, hk, 0, 1024, 2048)
    assert cls["T"] == [31, 16] and cls["TC"] == [7, 0] and cls["wg"][:2] == [0, 224]
    assert counts[1, 0, 0] == 1


def test_more_fronts_than_classes_the_last_class_takes_the_rest():
    # tile rows falling by more than 30 % per front (k = m: T = (m - 64) / 64 after the first panel), then fronts that end
    # inside the panel and have one tile row more than the front before them: one class each until the table is full
    Ts = [300, 200, 130, 90, 60, 40, 27, 18, 12, 8, 5, 3, 2, 1]
    hm = [64 + 64 * T for T in Ts] + [129, 128, 128, 127, 100, 99]
    hk = [64 + 64 * T for T in Ts] + [1, 64, 1, 64, 1, 99]
    counts, cls = check_cover(0, hm, hk, 0, 64, INT_MAX)
    assert cls["ncls"] == MAXCLS
    for kb, klen, col_lim in ((0, 128, INT_MAX), (0, 64, 128), (0, 256, 512)):
        check_cover(0, hm, hk, kb, klen, col_lim)
    check_cover(1, hm, hk, 0, 256, 512)


def test_fronts_without_columns_in_the_panel_and_empty_regions():
    # k <= kb: nothing; m == k: an empty region after the last panel; a front whose region is one row
    hm = [900, 800, 700, 600, 129, 65]
    hk = [100, 800, 64, 600, 128, 1]
    for kb, klen, col_lim in ((64, 64, INT_MAX), (0, 64, INT_MAX), (0, 128, INT_MAX), (64, 128, 256), (0, 512, 1024)):
        counts, _ = check_cover(0, hm, hk, kb, klen, col_lim)
        for f in range(len(hm)):
            if hk[f] <= kb:
                assert counts[f].sum() == 0
    check_cover(1, hm, hk, 0, 256, 512)
    check_cover(1, [800, 600], [800, 600], 0, 256, 512)             # far launch with nothing right of the block: empty
    counts, cls = check_cover(0, [128], [128], 64, 64, INT_MAX)     # one front, last panel: the region is empty
    assert counts.sum() == 0


def test_random_launches_of_every_shape():
    rng = np.random.default_rng(2024)
    ntried = 0
    for it in range(900):
        u_block = int(rng.choice([256, 512, 1024]))
        count = int(rng.integers(1, 24))
        kind = it % 3
        if kind == 0:                                   # wide spread of orders
            hm = rng.integers(129, 4000, count)
        elif kind == 1:                                 # near-equal orders around a class boundary
            base = int(rng.integers(600, 2200))
            hm = base - rng.integers(0, 160, count)
        else:                                           # few pivots, long update regions (dense rows)
            hm = rng.integers(200, 3000, count)
        hk = np.array([int(rng.integers(1, m + 1)) if rng.random() < 0.6 else int(rng.integers(1, min(m, 300) + 1)) for m in hm])
        hm, hk = hm.tolist(), hk.tolist()
        for uonly, m, k, kb, klen, col_lim in child.launch_shapes(hm, hk, u_block):
            if m:
                check_cover(uonly, m, k, kb, klen, col_lim)
                ntried += 1
    assert ntried > 5000


# ---- the chain lists of analysed factors ---------------------------------------------------------------------------------------
def _levels_cover(F, u_blocks=(256, 384, 512, 1024)):
    levels = child.chain_levels(F)
    assert levels
    nl = 0
    for hm, hk in levels.values():
        for u_block in u_blocks:
            for uonly, m, k, kb, klen, col_lim in child.launch_shapes(hm, hk, u_block):
                if m:
                    check_cover(uonly, m, k, kb, klen, col_lim)
                    nl += 1
    return nl


@pytest.mark.parametrize("name", ["laplacian_2d_1000", "stencil21_2d_200", "laplacian_3d_30"])
def test_chain_lists_of_mesh_factors(name):
    n, cp, ri, v = {"laplacian_2d_1000": lambda: workloads.laplacian_2d(1000),
                    "stencil21_2d_200": lambda: workloads.stencil21_2d(200),
                    "laplacian_3d_30": lambda: workloads.laplacian_3d(30)}[name]()
    assert _levels_cover(Factor(n, cp, ri)) > 0


@pytest.mark.parametrize("seed,n,dens", [(2, 300, 0.03), (3, 1500, 0.004), (4, 2500, 0.02)])
def test_chain_lists_of_random_spd_patterns(seed, n, dens):
    """the patterns of test_chol_gpu.py::test_random_spd_parity that have big fronts"""
    n, cp, ri, v = child.random_spd(n, dens, seed, 1.0 + seed)
    _levels_cover(Factor(n, cp, ri))


@pytest.mark.parametrize("name", ["bcsstk13", "bcsstk24"])
def test_chain_lists_of_the_reference_test_matrices(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    _levels_cover(Factor(int(z["n"]), z["colptr"], z["rowind"]))


@pytest.mark.parametrize("name", child.ALL_MATRICES)
def test_chain_lists_of_the_schedule_test_matrices(name):
    n, cp, ri, v, perm, opts = child.matrix(name)
    _levels_cover(Factor(n, cp, ri, "L", perm, opts))


def test_gadgets_give_the_intended_fronts_and_classes():
    """The GPU schedule tests rely on these: level 1 holds exactly the listed fronts, and their launches form the overlapping
    class layouts (a triangular class of 16+ tile rows behind another class, padding in front of it)."""
    for name, fronts in child.GADGETS.items():
        n, cp, ri, v, perm, opts = child.matrix(name)
        levels = child.chain_levels(Factor(n, cp, ri, "L", perm, opts))
        assert sorted(levels) == [0, 1], name
        assert list(zip(*levels[1])) == fronts, name
    for launch in ((0, [2100, 1500], [812, 1100], 0, 512, 1024), (0, [1020, 1019], [127, 1], 0, 128, INT_MAX),
                   (0, [1276, 1275], [383, 257], 256, 128, INT_MAX)):
        _, cls = cover(*launch)
        tiles0 = cls["T"][0] * cls["TC"][0] if cls["TC"][0] else cls["T"][0] * (cls["T"][0] + 1) // 2
        assert cls["ncls"] == 2 and cls["T"][1] >= 16 and cls["TC"][1] == 0, launch
        assert cls["wg"][1] > tiles0, launch                     # padding ids in front of the XCD-numbered class
