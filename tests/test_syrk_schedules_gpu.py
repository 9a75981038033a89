"""Every schedule of the big fronts' trailing update against the CPU oracle, each setting in a process of its own
(syrk_schedule_child.py: the knobs are read once per process).  The child checks the factor entries, diag(), the solves of
sys 0-8, the residual and the bits of an eager, a captured and a replayed factorisation; here the launch counters
(kvx_dbg_syrk_counts) prove that the forced kernel or schedule ran.  test_chol_gpu.py::test_syrk128_variant_parity runs the
128-tile kernel and the two-level blocking the same way."""
import pytest

from kvxopt_amd import _lib

import syrk_schedule_child as child

pytestmark = pytest.mark.gpu

BIG = 10**12
SETTINGS = [("default", {})]
for _u in (256, 512, 1024):
    SETTINGS += [("blocked_u%d" % _u, {"KVX_BLOCKED_GF": 0, "KVX_U_BLOCK": _u}),
                 ("blocked_u%d_one_stream" % _u, {"KVX_BLOCKED_GF": 0, "KVX_U_BLOCK": _u, "KVX_U_STREAM": 0}),
                 ("blocked_u%d_far_wgs7" % _u, {"KVX_BLOCKED_GF": 0, "KVX_U_BLOCK": _u, "KVX_FAR_WGS": 7})]
SETTINGS += [("pairs_always", {"KVX_PAIR_TILES": 0}), ("pairs_never", {"KVX_PAIR_TILES": BIG}),
             ("lds_always", {"KVX_SYRK_LDS_TILES": 0}), ("lds_never", {"KVX_SYRK_LDS_TILES": BIG}),
             ("round3", {"KVX_DEFER_U": 0, "KVX_BLOCKED_GF": 0}),      # (the blocked schedule everywhere, but for KVX_DEFER_U=0)
             ("direct", {"KVX_SYRK_DIRECT": 1})]


def expect(name, res):
    """what the counters of a setting must show (summed over the matrices, and per gadget where the gadget forces it)"""
    t = {c: child.total(res, c) for c in child.COUNTERS}
    g = {m: res[m]["counts"] for m in child.GADGETS}
    others = ("t64_grid", "t128_grid", "t128_panel", "outer")
    if name == "default":
        assert t["t64_cls"] > 0 and t["lds_far"] == 0, t
    elif name.startswith("blocked_u"):
        assert t["lds"] > 0 and t["lds_far"] > 0, t
        assert all(g[m]["lds_far"] > 0 for m in g), g                           # far launches of every gadget
        assert g["gadget_near512"]["lds"] > 0, g          # near launches: its level 1 has more pivot columns than any block
        if name.endswith("_one_stream"):
            assert t["far_side"] == 0, t
        else:
            assert t["far_side"] > 0, t
        if name.endswith("_far_wgs7"):
            assert t["lds_far_stride"] > 0, t
        else:
            assert t["lds_far_stride"] == 0, t
    elif name == "pairs_always":
        assert t["t128_cls"] > 0 and g["gadget_pair0"]["t128_cls"] > 0 and g["gadget_pair256"]["t128_cls"] > 0, (t, g)
    elif name == "pairs_never":
        assert t["t128_cls"] == 0 and t["t128_grid"] == 0, t
    elif name == "lds_always":
        assert t["lds"] > 0 and t["t64_cls"] == 0 and t["t128_cls"] == 0, t
    elif name == "lds_never":
        assert t["lds"] == 0 and t["t64_cls"] > 0, t
    elif name == "round3":
        assert t["lds_far"] == 0 and t["far_side"] == 0 and t["t64_cls"] > 0, t
    elif name == "direct":
        assert t["t64_grid"] > 0, t
        assert all(t[c] == 0 for c in ("t64_cls", "t128_cls", "lds", "lds_far", "t128_panel", "outer")), t
    if name != "direct":
        assert all(t[c] == 0 for c in others), (name, t)


def test_every_trailing_update_schedule_against_the_oracle(tmp_path):
    _lib.require_device()
    cache = str(tmp_path)
    for m in child.ALL_MATRICES:
        child.prepare(m, cache)
    out = {}
    for name, setting in SETTINGS:
        out[name] = child.run_setting(setting, child.ALL_MATRICES, cache)
        expect(name, out[name])
    # the far updates on the chain's stream, and walked by 7 resident workgroups: the same tiles by the same kernel, the same bits
    for u in (256, 512, 1024):
        base = out["blocked_u%d" % u]
        for var in ("blocked_u%d_one_stream" % u, "blocked_u%d_far_wgs7" % u):
            for m in child.ALL_MATRICES:
                assert out[var][m]["digest"] == base[m]["digest"], (var, m)
