"""CPU tests of the case list of tests/test_gpu_grad_extended.py (tests/grad_cases.py): no GPU.

* the plans restated in grad_cases are the ones of the kernel sources;
* for every case: the bound of EVERY segment of the pinned segmentation, by the bound its backward sweep plans with, lies in the
  band of the scheme the case claims, and every segment holds at least two slices (a one-slice segment of odd index would see
  amplitudes below 1 and plan another scheme);
* for every problem: the yardstick e_cpu -- the worst error of the oracle's gradient and of a scipy route against the
  long-double reference -- and the conditions that keep it honest: every slice inside the radius of Pade-13, e_cpu <= 1e-13, and
  the largest reference entry at least 1e-3 of ||U_bar||_F dt max_k ||h_k||_F.  Each reference within 30 s.  The table is printed.
"""
import json
import os
import re
import time

import numpy as np
import pytest

import extended_ref as x
import grad_cases as gc
import pwc_cases as pc
from oracle import c3_oracle as o

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "c3_amd", "csrc")
E_CPU_MAX = 1e-13
FLOOR = 1e-3  # tests/test_gpu_smalld_grad_segments.py
REF_SECONDS = 30.0


def test_plans_restate_the_sources():
    src = lambda f: open(os.path.join(CSRC, f)).read()
    sd, md, rg = src("c3p_smalld.hip"), src("c3p_midd.hip"), src("c3p_regrg_body.inc")
    assert int(re.search(r"constexpr int SDG_MAXS = (\d+);", sd).group(1)) == gc.SDG_MAXS
    assert "static constexpr int MAXS = (NIG + 1) / 2 >= 3 ? 1 : 2;" in md
    assert [gc.midd_maxs(D) for D in (13, 16, 17, 24, 25, 32, 33, 36, 40)] == [2, 2, 2, 2, 2, 2, 1, 1, 1]
    th = re.search(r"const double th\[4\] = \{([^}]*)\}", rg).group(1)
    assert tuple(float(t) for t in th.split(",")) == gc.REGRG_THETA
    assert "const int cost = 3 * Ji + 3 * si;" in rg and "if (cost < best) best = cost" in rg
    # the cost rule at a few norms, by hand: a degree up costs two squarings
    assert [gc.regr_plan(n) for n in (0.05, 0.06, 0.15, 0.25, 0.33, 0.5, 0.8, 1.0, 1.4)] == [(8, 0), (8, 1), (8, 2), (12, 0), (8, 3), (12, 1), (8, 4), (12, 2), (8, 5)]


@pytest.mark.parametrize("c", gc.CASES, ids=gc.CASE_IDS)
def test_every_segment_lies_in_the_claimed_band(c):
    p = c.problem
    k = gc.key_of(c)
    inp = gc.grad_inputs(k)
    # a pure function of the case
    again = gc.grad_inputs.__wrapped__(k)
    for a, b in zip(inp, again):
        assert (a is None and b is None) or (np.asarray(a).tobytes() == np.asarray(b).tobytes())
    # the pinned segmentation: at least two slices everywhere
    segs = gc.segments(p.N, c.S)
    assert min(n1 - n0 for n0, n1 in segs) >= 2, (c.S, p.N)
    opts = dict(c.opts)
    if "smalld_segments" in opts:
        assert opts["smalld_segments"] == c.S
    if "valu_grad_segments" in opts:
        assert opts["valu_grad_segments"] == c.S
    if "grad_target" in opts:
        assert opts["grad_target"] == p.B and c.S == 1
    if c.family in ("mdg_general", "mdg_xg"):
        assert c.S == max(1, min((1024 if (p.D * p.D if p.lind else p.D) <= 32 else 512) // p.B, p.N // 8))  # midd_grad_segments
    if c.family in ("hbg_reg", "tiled"):
        assert c.S == 1 and p.N // 4 <= 1  # lind_regr_segments: smax = N / 4; the tiled sweep has no segments
    # the bound that fixed dt reaches its target in the largest sample
    own = gc.segment_bounds(c._replace(family={"col": "sdg_real", "sum": "mdg_pair", "sumT": "mdg_general", "hbT": "hbg_small", "slice": "valu", "seg": "sdg_xg"}[c.bound]), inp)
    assert abs(max(s[3] for s in own) - c.target) <= 1e-9 * c.target, (max(s[3] for s in own), c.target)
    # every segment in the claimed band
    seen = set()
    for b, n0, n1, bound, nsym in gc.segment_bounds(c, inp):
        if p.ham == "mixed" and b == 1:
            continue
        if c.family == "valu" and n0 % 2:
            # planned slice by slice: the claim is that of the slices with |c_k| = 1 (the even ones); an odd slice may take fewer squarings
            # (odd next to even counts inside one segment: t18_pair swaps the roles of its buffers once per squaring)
            assert bound <= c.target * (1 + 1e-12)
            continue
        seen.add(gc.grad_scheme_of(c.family, bound, nsym, p.D, c.degree))
    assert seen == {c.scheme}, (c.id, seen, c.scheme)
    if c.handover:
        fam, scheme = c.handover
        seen = {gc.grad_scheme_of(fam, bound, nsym, p.D) for b, n0, n1, bound, nsym in gc.segment_bounds(c, inp, fam) if p.ham != "mixed" or b == 1}
        assert seen == {scheme}, (c.id, seen, scheme)
    assert (c.scheme == "handover") == (c.handover is not None and p.ham != "mixed")
    if p.ham == "mixed":
        assert np.abs(inp.hks[1].imag).max() > 0 and np.abs(inp.hks[0].imag).max() == 0 and np.abs(inp.hks[2].imag).max() == 0


_TABLE = []


@pytest.mark.parametrize("k", gc.KEYS, ids=[[c.id for c in gc.CASES if gc.key_of(c) == k][0] for k in gc.KEYS])
def test_yardstick_is_honest(k):
    p = k.problem
    inp = gc.grad_inputs(k)
    X = pc.slice_generators(inp, p.lind is not None)
    worst = max(x.norm1(X[b, n]) for b in range(X.shape[0]) for n in range(X.shape[1]))
    assert worst < o.PADE_THETA[4], worst
    t0 = time.perf_counter()
    ref = gc.grad_reference(k)
    secs = time.perf_counter() - t0
    ids = [c.id for c in gc.CASES if gc.key_of(c) == k]
    line = (f"YARDSTICK {ids[0]} (+{len(ids) - 1}) max||X_n||_1={worst:.3g} e_cpu={ref.e_cpu:.3e} (oracle {ref.e_oracle:.3e}, scipy {ref.e_scipy:.3e})"
            + (f" e_cpu_phase={ref.e_cpu_ph:.3e}" if ref.e_cpu_ph is not None else "") + f" floor={ref.floor:.3g} reference {secs:.1f} s")
    print("\n" + line)
    _TABLE.append(line)
    assert 0.0 < ref.e_cpu <= E_CPU_MAX
    assert ref.e_cpu_ph is None or 0.0 < ref.e_cpu_ph <= E_CPU_MAX
    assert ref.floor >= FLOOR
    assert secs < REF_SECONDS


def test_case_list_reaches_every_band_edge():
    """A pair of cases straddles each radius at (1 -+ 1e-3)."""
    by_id = {c.id: c for c in gc.CASES}
    pairs = [f"sdg-real-D9-%s-{e:g}" for e in (0.83, 1.85, 3.7, 7.4, 14.8)] + [f"sdg-herm-D9-%s-{e:g}" for e in (1.13, 2.26)]
    pairs += [f"mdg-real-D13-%s-{e:g}" for e in (1.85, 3.7, 7.4)] + ["mdg-real-D36-%s-3.7"] + [f"lindg-regr-D7-%s-{e:g}" for e in gc.REGRG_THETA]
    for pat in pairs:
        a, b = by_id[pat % "below"], by_id[pat % "above"]
        assert abs(b.target / a.target - (1 + x.EDGE) / (1 - x.EDGE)) < 1e-12
        # (the cost rule of regr_grad_kernel does not switch at 0.816 and 1.49: a tie goes to the lower degree on both sides)
        assert a.scheme != b.scheme or pat.startswith("lindg-regr-D7-%s-") and a.scheme in ("ty8+4", "ty8+5")


def test_every_kernel_class_has_a_recorded_launch_log(golden_dir):
    """tests/golden/grad_extended_kernels.json (launch logs recorded on the MI355X) names exactly the kernel classes of the cases;
    a hand-over class shows both sweeps."""
    recorded = json.load(open(os.path.join(golden_dir, "grad_extended_kernels.json")))
    assert sorted(recorded) == sorted({c.kernel for c in gc.CASES})
    assert all(isinstance(v, str) and ".hip: " in v for v in recorded.values())
    for c in gc.CASES:
        if c.scheme == "handover":
            assert "grad_real_kernel" in recorded[c.kernel] and ("smalld_grad_kernel" in recorded[c.kernel] or "midd_grad_kernel" in recorded[c.kernel]), c.kernel


def test_expected_failures_are_whole_groups():
    """The expected failures of tests/test_gpu_grad_extended.py are declared per group (`grad_cases.group_of`: kernel class, scheme, position
    of the bound in its squaring band, variant), and the case ids listed under a group are exactly the members of that group."""
    from test_gpu_grad_extended import OVER_THE_BAR, OVER_THE_BAR_GROUPS

    members = {}
    for c in gc.CASES:
        members.setdefault(gc.group_of(c), set()).add(c.id)
    for group, listed in OVER_THE_BAR_GROUPS.items():
        assert group in members, group
        assert set(listed) == members[group], (group, sorted(listed), sorted(members[group]))
    assert len(OVER_THE_BAR) == sum(len(v) for v in OVER_THE_BAR_GROUPS.values())
    # positions as intended: the pair members sit at the ends of their bands, the 10 %-inside targets in the middle
    by_id = {c.id: c for c in gc.CASES}
    assert gc.band_position(by_id["sdg-real-D9-above-1.85"]) == "lo" and gc.band_position(by_id["sdg-real-D9-below-3.7"]) == "hi"
    assert gc.band_position(by_id["sdg-real-D9-K2-mm8+1"]) == "mid" and gc.band_position(by_id["sdg-real-D9-K2-mm8+0"]) == "mid"

