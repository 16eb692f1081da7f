"""GPU tests of the PWC signal gradients -- `propagate_batch_vjp`, `propagate_batch_lindblad_vjp`, `propagate_batch_goal_vjp`,
`propagate_per_slice_vjp` -- against extended precision (tests/extended_ref.py: `pwc_signal_gradient_ld`), sweep by sweep and
scheme by scheme.  -m gpu.

The backward sweeps carry polynomial machinery of their own (the hand-written reverse mode through the degree-6 / degree-8 pairs
with the stacks of their squaring adjoints, the forward-mode T18 pairs, the Taylor pairs of the Hermitian-basis sweep) which the
propagator test never touches, and every other gradient test compares with the double-precision oracle at 1e-10.  One test = one
case of tests/grad_cases.py = one library call and one reference:

* the kernel instances of the call (`_lib.last_kernel_detail()`) are the recorded ones of the case's class
  (tests/golden/grad_extended_kernels.json: launch logs of these very calls); a hand-over case shows both sweeps;
* the same call again returns the same bits;
* a hard backstop outside any expected failure: max|g_b - ref_b| / max|ref_b| <= 1e-12 for every sample;
* the bar: that ratio <= 8 e_cpu, e_cpu the worst error over the samples of two double-precision CPU routes against the same
  reference (the oracle's gradient; scipy's expm / expm_frechet under double prefix products).  8 = `extended_ref.CHAIN_FACTOR`,
  carried over: the device pairs may take up to three more squarings than Pade-13, and squaring a (value, derivative) pair at most
  doubles the first-order bound.  Not tuned to what the kernels return.  The fused goal: gradient and phase gradient, each against
  its own long-double value and its own e_cpu.

tests/test_grad_extended_ref.py asserts (without a GPU) that every segment's bound lies in the band the case claims and the
conditions that keep e_cpu honest.  Cases over the bar are strict expected failures, declared as whole groups (`OVER_THE_BAR_GROUPS`) that the
same CPU file checks against the case list; measured: 114 inside the bar (0.4 ... 7.5 x e_cpu), 43 over it (8.2 ... 97).  Every figure is printed before it is asserted (pytest -s shows the table DESIGN section 3
records).
"""
import json
import os

import numpy as np
import pytest

import extended_ref as x
import grad_cases as gc

pytestmark = pytest.mark.gpu

_KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_extended_kernels.json")
KERNELS = json.load(open(_KERNELS))
BACKSTOP = 1e-12  # an order above the worst figure DESIGN 5.6 records against the oracle (8.6e-14)


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


class GradBarExceeded(AssertionError):
    """The 8 e_cpu bar itself (an expected failure covers nothing else: kernel instances, repeatability and the backstop still fail)."""


# Groups that EXCEED 8 e_cpu on the MI355X: group (`grad_cases.group_of`: kernel class, scheme, position of the bound in its squaring band,
# variant -- all computable without a GPU) -> {case id: e_device / e_cpu as measured}.  Only WHOLE groups: tests/test_grad_extended_ref.py
# asserts that the ids listed under a group are exactly its members.  DESIGN section 3 has the cause.  The bar is not tuned to them: they stay
# strict expected failures until the maintainers decide.
OVER_THE_BAR_GROUPS = {
    ('sdg-real-D5', 'mm8+1', 'mid', ''): {"sdg-real-D5-K2-mm8+1": 12, "sdg-real-D5-K3-mm8+1": 18.6},
    ('sdg-real-D5', 'mm8+2', 'mid', ''): {"sdg-real-D5-K2-mm8+2": 18.1},
    ('sdg-real-D9', 'mm8+1', 'mid', ''): {"sdg-real-D9-K2-mm8+1": 13.6, "sdg-real-D9-K3-mm8+1": 15.3},
    ('sdg-real-D9', 'mm8+2', 'mid', ''): {"sdg-real-D9-K2-mm8+2": 32.7},
    ('sdg-real-D9', 'mm8+3', 'mid', 'cancel'): {"sdg-real-D9-K2-mm8+3": 8.21},
    ('sdg-real-D3', 'mm8+1', 'mid', ''): {"sdg-real-D3-mm8+1": 11.2},
    ('sdg-real-D4', 'mm8+2', 'mid', ''): {"sdg-real-D4-mm8+2": 25.8},
    ('sdg-real-D8', 'mm8+1', 'mid', ''): {"sdg-real-D8-mm8+1": 29.4},
    ('sdg-real-D12', 'mm8+2', 'mid', ''): {"sdg-real-D12-mm8+2": 23.9},
    ('sdg-real-D9', 'mm8+1', 'hi', ''): {"sdg-real-D9-below-3.7": 14.1},
    ('sdg-real-D9', 'mm8+2', 'lo', ''): {"sdg-real-D9-above-3.7": 29.6},
    ('sdg-real-D9', 'mm8+2', 'hi', 'cancel'): {"sdg-real-D9-below-7.4": 15},
    ('sdg-real-D9', 'mm8+3', 'hi', 'cancel'): {"sdg-real-D9-below-14.8": 31},
    ('sdg-mixed-D9-trace-phase', 'mm8+0>t18+1', 'mid', ''): {"sdg-mixed-D9-trace-phase": 11.7},
    ('sdg-real-D9-per-sample-h0', 'mm6+0', 'mid', 'per_sample_h0'): {"sdg-real-D9-per-sample-h0-mm6+0": 10.4},
    ('sdg-herm-D9', 't18+2', 'mid', ''): {"sdg-herm-D9-t18+2": 11.1},
    ('sdg-herm-D9-trace', 't18+1', 'mid', ''): {"sdg-herm-D9-trace": 9.73},
    ('sdg-herm-D9', 't18+1', 'hi', ''): {"sdg-herm-D9-below-2.26": 11},
    ('sdg-herm-D9', 't18+2', 'lo', ''): {"sdg-herm-D9-above-2.26": 20.5},
    ('mdg-real-D13', 'mm8+1', 'mid', ''): {"mdg-real-D13-mm8+1": 18.1},
    ('mdg-real-D13', 'mm8+2', 'mid', ''): {"mdg-real-D13-mm8+2": 58.2},
    ('mdg-real-D16', 'mm8+1', 'mid', ''): {"mdg-real-D16-mm8+1": 24.2},
    ('mdg-real-D16', 'mm8+2', 'mid', ''): {"mdg-real-D16-mm8+2": 75.3},
    ('mdg-real-D17', 'mm8+1', 'mid', ''): {"mdg-real-D17-mm8+1": 12.2},
    ('mdg-real-D17', 'mm8+2', 'mid', ''): {"mdg-real-D17-mm8+2": 50.3},
    ('mdg-real-D27', 'mm8+1', 'mid', ''): {"mdg-real-D27-mm8+1": 29.1},
    ('mdg-real-D27', 'mm8+2', 'mid', ''): {"mdg-real-D27-mm8+2": 96.9},
    ('mdg-real-D36', 'mm8+1', 'mid', ''): {"mdg-real-D36-mm8+1": 26.5},
    ('mdg-real-D40', 'mm8+0', 'mid', ''): {"mdg-real-D40-mm8+0": 9.34},
    ('mdg-real-D40', 'mm8+1', 'mid', ''): {"mdg-real-D40-mm8+1": 28.2},
    ('mdg-real-D13', 'mm8+1', 'lo', ''): {"mdg-real-D13-above-1.85": 9.28},
    ('mdg-real-D13', 'mm8+1', 'hi', ''): {"mdg-real-D13-below-3.7": 13.7},
    ('mdg-real-D13', 'mm8+2', 'lo', ''): {"mdg-real-D13-above-3.7": 89.1},
    ('mdg-real-D13', 'mm8+2', 'hi', 'cancel'): {"mdg-real-D13-below-7.4": 19.5},
    ('mdg-real-D13-handover', 'handover>t18+3', 'mid', 'cancel'): {"mdg-real-D13-above-7.4": 22.4},
    ('mdg-real-D36', 'mm8+1', 'hi', ''): {"mdg-real-D36-below-3.7": 19.9},
    ('mdg-real-D36-handover', 'handover>t18+2', 'mid', ''): {"mdg-real-D36-above-3.7": 23.3},
    ('mdg-herm-D13', 't18+2', 'mid', ''): {"mdg-herm-D13-t18+2": 9.14},
    ('lindg-regr-D8', 'ty8+3', 'mid', ''): {"lindg-regr-D8-degree8": 8.89},
    ('lindg-regr-D7', 'ty8+5', 'mid', ''): {"lindg-regr-D7-below-1.49": 15.5, "lindg-regr-D7-above-1.49": 9.29},
}
OVER_THE_BAR = {cid: r for members in OVER_THE_BAR_GROUPS.values() for cid, r in members.items()}


def _param(c):
    if c.id not in OVER_THE_BAR:
        return pytest.param(c, id=c.id)
    reason = f"e_device / e_cpu = {OVER_THE_BAR[c.id]:g} measured on the MI355X (bar {x.CHAIN_FACTOR:g})"
    return pytest.param(c, id=c.id, marks=pytest.mark.xfail(strict=True, raises=GradBarExceeded, reason=reason))


@pytest.mark.parametrize("c", [_param(c) for c in gc.CASES])
def test_gradient_against_extended_precision(prop, c):
    from c3_amd import _lib

    p = c.problem
    k = gc.key_of(c)
    inp = gc.grad_inputs(k)
    g, gph, detail = gc.call_case(prop, _lib, c, inp)
    print(f"\nKERNEL {c.kernel} | {detail}")
    ref = gc.grad_reference(k)
    assert g.shape == ref.g.shape and g.dtype == (np.complex128 if p.per_slice else np.float64)
    e = x.grad_err(g, ref.g)
    print(f"GRAD {c.id} class={c.kernel} scheme={c.scheme}{'>' + c.handover[1] if c.handover else ''} e_device={e:.3e} e_cpu={ref.e_cpu:.3e} "
          f"(oracle {ref.e_oracle:.3e}, scipy {ref.e_scipy:.3e}) ratio={e / ref.e_cpu:.3g}")
    e_ph = None
    if c.goal:
        assert gph.shape == ref.gph.shape and gph.dtype == np.float64
        e_ph = x.grad_err(gph, ref.gph)
        print(f"GRAD-PHASE {c.id} class={c.kernel} scheme={c.scheme} e_device={e_ph:.3e} e_cpu={ref.e_cpu_ph:.3e} ratio={e_ph / ref.e_cpu_ph:.3g}")
    assert detail == KERNELS[c.kernel], (c.kernel, detail)
    # the same call again gives the same bits
    g2, gph2, detail2 = gc.call_case(prop, _lib, c, inp)
    assert detail2 == detail
    assert x.same_bits(g, g2)
    if c.goal:
        assert x.same_bits(gph, gph2)
    assert e <= BACKSTOP, (c.id, e)
    assert e_ph is None or e_ph <= BACKSTOP, (c.id, e_ph)
    try:
        x.check_grad(g, ref.g, ref.e_cpu)
        if c.goal:
            x.check_grad(gph, ref.gph, ref.e_cpu_ph)
    except AssertionError as err:
        raise GradBarExceeded(str(err)) from err


def test_k0_gradient_call_is_refused(prop):
    """K = 0: there is no control line and no signal gradient; the gradient entry refuses the sizes (an error, never a silent empty result
    or a launch with K = 0 tables)."""
    from c3_amd import _lib
    from c3_amd._lib import C3PropError

    c = gc.K0_CASE
    inp = gc.grad_inputs(gc.key_of(c))
    assert inp.hks.shape == (0, 9, 9) and inp.signals.shape == (3, 0, gc.SD_N)
    with pytest.raises(C3PropError, match="bad sizes"):
        gc.call_case(prop, _lib, c, inp)
