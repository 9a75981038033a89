"""The triangular sweeps over the big fronts (m > 128 or k > 64) at their block and row edges, on the designed systems of
chol_big_solve_cases.py (test_chol_big_solve_cpu.py pins the designs and the expected launches on the host).  Every (setting, case)
is one child process (chol_big_solve_child.py, which holds the routings and the criteria): KVX_FWD_NARROW_WGS, the threshold
between the 64-row and the 256-row form of the forward step, is read once per process.

  default   no knob: the 64-row form wherever a level stays within 512 workgroups -- every case but crowd257
  rows256   KVX_FWD_NARROW_WGS=0: never the 64-row form; from 64 right-hand sides on the blocks of eight in the forward sweep too

The two settings add a row's partial sums in different associations (sixteen in sequence, four paired): their bits are not
compared, each meets the bounds.  One child at a time, each under its own time limit; a child that dies by a signal or at its
time limit fails its item and no further child is started."""
import subprocess

import pytest

import chol_big_solve_cases as bc
import chol_big_solve_child as child
from kvxopt_amd import _lib

pytestmark = pytest.mark.gpu

ITEMS = [("default", c.name) for c in bc.CASES] + [("rows256", c.name) for c in bc.CASES if c.name not in bc.CROWDS]
ENOUGH = (("default", "super3"), ("rows256", "super3"))      # between them every one of the 17 kernels
HITS = {s: {c: 0 for c in bc.COUNTERS} for s in child.SETTINGS}
WORST, SECONDS, RAN = {}, {}, set()
DEAD = {"cases": set(), "stop": None}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def run_item(setting, name):
    if DEAD["stop"]:
        pytest.fail("no further child: %s" % DEAD["stop"])
    if name in DEAD["cases"]:
        pytest.fail("no further child for %s: an earlier one failed to finish" % name)
    try:
        rc, res, tail = child.run_child(setting, name)
    except subprocess.TimeoutExpired:
        DEAD["stop"] = "the child of (%s, %s) ran into its time limit of %d s" % (setting, name, child.TIMEOUT)
        pytest.fail(DEAD["stop"])
    if rc < 0 or rc in (124, 134, 137, 139):
        DEAD["stop"] = "the child of (%s, %s) died with status %d" % (setting, name, rc)
        pytest.fail(DEAD["stop"] + "\n" + tail)
    if rc != 0 or res is None:
        DEAD["cases"].add(name)
        pytest.fail("child of (%s, %s): status %d\n%s" % (setting, name, rc, tail))
    print(setting, name, res["seconds"], {k: round(v, 3) for k, v in sorted(res["ratios"].items())})
    RAN.add((setting, name))
    SECONDS[(setting, name)] = res["seconds"]["all"]
    for k, v in res["hits"].items():
        HITS[setting][k] += v
    for k, v in res["ratios"].items():
        WORST[(setting, k)] = max(WORST.get((setting, k), (0.0, "")), (v, name))
    return res


@pytest.mark.parametrize("setting,name", ITEMS)
def test_case(setting, name):
    res = run_item(setting, name)
    assert res["narrow_wgs"] == (0 if setting == "rows256" else 512)
    assert not res["errors"], (setting, name, res["errors"])
    sets = child.nrhs_sets(name)
    assert res["replays"] == 3 * (len(sets["a"]) + len(sets["b"])), (setting, name, "third calls (routings a, b) that replayed a graph", res["replays"])
    h = res["hits"]
    if setting == "rows256":
        assert h["fwd_first64"] == h["fwd_next64"] == 0 and h["fwd_first256"] > 0 and h["fwd_mr_first_diag"] > 0, h
    elif name == "crowd257":        # 257 roots of two 64-row workgroups each: past the threshold without any knob
        assert h["fwd_first256"] > 0 and h["fwd_mr_first_diag"] > 0 and h["fwd_mr_first_rows"] > 0 and h["fwd_first64"] == 0, h
    else:
        assert h["fwd_first64"] > 0 and all(h[k] == 0 for k in bc.COUNTERS if k.endswith("256") or k.startswith("fwd_mr")), h
    assert all(h[k] > 0 for k in ("bwd_init", "bwd_step", "bwd_mr_init", "bwd_mr_step_diag", "wide_fwd_asm", "wide_bwd_head")), h


@pytest.fixture(scope="module")
def hits():
    """the launches seen over the module; selected alone, the test below gets the children of ENOUGH run here"""
    for setting, name in ENOUGH:
        if (setting, name) not in RAN:
            test_case(setting, name)
    return HITS


def test_every_big_solve_kernel_ran(hits):
    """summed over the children, every launch site of the four big-front sweep launchers was taken"""
    print("largest ratio to the bound per (setting, routing/sys): (ratio, case)")
    for k, v in sorted(WORST.items()):
        print("   %-8s %-8s %.3f  %s" % (k[0], k[1], v[0], v[1]))
    print("seconds per child:", {"%s/%s" % k: v for k, v in sorted(SECONDS.items())})
    total = {c: sum(hits[s][c] for s in hits) for c in bc.COUNTERS}
    assert all(total[c] > 0 for c in bc.COUNTERS), {c: v for c, v in total.items() if v == 0}
    assert all(hits["rows256"][c] == 0 for c in ("fwd_first64", "fwd_next64")), hits["rows256"]
