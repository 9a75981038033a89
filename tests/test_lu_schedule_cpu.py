"""The factor-side level schedule of the sparse LU plan (lu_symbolic.hpp LuLevelSched), read on the CPU through kvx_dbg_lu_schedule:
the launches of LDS fronts and the pivot blocks of the blocked part that a numeric pass runs, checked against the dumped (m, k)
lists alone and against the Python model of lu_class_child (lds_T, block_width, panel_steps).

Order 4100 -- the smallest front with more than 4096 rows, the only kind that sets lds_work -- is not built here: its analysis
is that of a 16.8 M-entry matrix.  lds_work = 1 stays as uncovered as k_lub_panel is on the GPU (test_lu_classes_gpu.py)."""
import numpy as np
import pytest

from kvxopt_amd import _lib
from kvxopt_amd.lu import LuSymbolic

import lu_class_child as child

CLASSES = (16, 32, 48, 64, 88, 112)
CASES = ["mixeda", "many20a", "two_classesa", "d112a", "d113a", "d1024a", "d1056a", "d2080a", "bp_800"]


def schedule(name):
    """name -> levels: dicts with fronts [(m, k)], lds [(first, count, class, side)], big (first, count, bm, bk), steps [(jb, width, lds_work)]"""
    n, cp, ri, v = child.case_matrix(name)
    sym = LuSymbolic(n, cp, ri, v)
    need = _lib.lib().kvx_dbg_lu_schedule(sym._h, None, 0)
    assert need > 0
    short = np.full(need - 1, -7, dtype=np.int64)
    assert _lib.lib().kvx_dbg_lu_schedule(sym._h, _lib.pi(short), need - 1) == need and np.all(short == -7)     # too short: untouched
    rec = np.full(need + 1, -7, dtype=np.int64)
    assert _lib.lib().kvx_dbg_lu_schedule(sym._h, _lib.pi(rec), need + 1) == need and rec[need] == -7
    rec = rec.tolist()
    pos = 1
    levels = []

    def take(count, width):
        nonlocal pos
        out = [tuple(rec[pos + i * width: pos + (i + 1) * width]) for i in range(count)]
        pos += count * width
        return out

    for _ in range(rec[0]):
        L = {}
        L["fronts"] = take(take(1, 1)[0][0], 2)
        L["lds"] = take(take(1, 1)[0][0], 4)
        L["big"] = take(1, 4)[0]
        L["steps"] = take(take(1, 1)[0][0], 3)
        levels.append(L)
    assert pos == need
    return n, levels


@pytest.mark.parametrize("name", CASES)
def test_schedule(name):
    n, levels = schedule(name)
    assert sum(k for L in levels for _, k in L["fronts"]) == n                    # every pivot in exactly one front
    if name != "bp_800":
        orders = child.case_blocks(name)[0]
        assert len(levels) == 1
        assert sorted(levels[0]["fronts"]) == sorted((m, m) for m in orders)
    else:
        assert len(levels) > 1
    for L in levels:
        fronts = L["fronts"]
        ms = [m for m, _ in fronts]
        nlds = sum(m <= child.LDS_M for m in ms)
        # 1. every front in exactly one launch or in the blocked part; the blocked part is exactly the fronts of m > 112
        first, count, bm, bk = L["big"]
        assert (first, count) == (nlds, len(fronts) - nlds)
        assert all(m <= child.LDS_M for m in ms[:nlds]) and all(m > child.LDS_M for m in ms[nlds:])
        # 2. the LDS launches: contiguous, in order, sides alternating from 0
        at = 0
        for i, (f, c, cls, side) in enumerate(L["lds"]):
            assert f == at and c > 0 and cls in CLASSES and side == i % 2
            at += c
        assert at == nlds
        if 0 < nlds <= 256:                                                       # one launch, sized for the largest front
            assert len(L["lds"]) == 1
            assert L["lds"][0][2] == min(c for c in CLASSES if c >= max(ms[:nlds]))
        elif nlds:                                                                # one launch per class
            assert len({cls for _, _, cls, _ in L["lds"]}) == len(L["lds"])
            for f, c, cls, _ in L["lds"]:
                assert all(child.lds_T(m) == child.lds_T(cls) for m in ms[f:f + c])
        # 3. maxima and pivot blocks of the blocked part
        big = fronts[nlds:]
        assert (bm, bk) == ((max(m for m, _ in big), max(k for _, k in big)) if big else (0, 0))
        want, jb = [], 0
        while jb < bk:
            want.append((jb, child.block_width(bm - jb), 0))                     # (no front here exceeds 4096 rows: lds_work = 0)
            jb += want[-1][1]
        assert L["steps"] == want
        widths = {"panel_reg%d" % w: sum(s[1] == w for s in L["steps"]) for w in (32, 16, 8)}
        assert dict(widths, panel_lds=0) == child.panel_steps(bm, bk)
    if name == "two_classesa":
        assert levels[0]["lds"] == [(0, 300, 48, 0), (300, 300, 16, 1)]          # (the list has its largest fronts first)
    if name == "many20a":
        assert levels[0]["lds"] == [(0, 600, 32, 0)]
    if name == "mixeda":                                                          # crosses the 32 -> 16 width switch
        assert levels[0]["big"] == (1, 3, 1500, 1500) and {s[1] for s in levels[0]["steps"]} == {16, 32}
    if name == "d2080a":                                                          # and the 16 -> 8 one
        assert {s[1] for s in levels[0]["steps"]} == {8, 16, 32}
