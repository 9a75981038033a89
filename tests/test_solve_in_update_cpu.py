"""The host's decision for the fused chain step (chol_internal.hpp solve_in_update, read through kvx_dbg_solve_in_update): single
panels over the whole trailing matrix, numbered over size classes, at most KVX_SOLVE_IN_UPDATE_TILES tiles -- never a
column-limited launch, a pair, a two-panel pass or the grid numbering of the sharded mode; 0 turns it off.  Needs no GPU."""
import itertools

from kvxopt_amd import _lib

INT_MAX = 2**31 - 1
COLS_PIVOT = 0x7FFFFFFE


def decide(knob, cls=1, pair=0, klen=64, col_lim=INT_MAX, tiles=1):
    return _lib.lib().kvx_dbg_solve_in_update(knob, cls, pair, klen, col_lim, tiles)


def test_threshold_is_inclusive_and_zero_is_off():
    assert decide(300, tiles=300) == 1 and decide(300, tiles=301) == 0 and decide(300, tiles=0) == 1
    assert decide(0, tiles=0) == 0 and decide(0, tiles=1) == 0
    assert decide(10**12, tiles=10**11) == 1               # 64-bit tile counts


def test_only_single_panels_over_the_whole_trailing_matrix_by_classes():
    for cls, pair, klen, col_lim in itertools.product((0, 1), (0, 1), (64, 128, 256, 384), (INT_MAX, COLS_PIVOT, 128, 192, 0)):
        want = 1 if (cls, pair, klen, col_lim) == (1, 0, 64, INT_MAX) else 0
        assert decide(10**9, cls, pair, klen, col_lim, 5) == want, (cls, pair, klen, col_lim)
