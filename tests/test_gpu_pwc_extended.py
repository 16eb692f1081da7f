"""GPU tests of the ASSEMBLED piecewise-constant propagators -- `propagate_batch` (c3p_pwc_unitary, c3p_pwc_lindblad), from
operators, amplitudes and dt to U -- against extended precision (tests/extended_ref.py: `pwc_ld`), scheme by scheme.  -m gpu.

tests/test_gpu_matrix_routines.py reaches the kernels through supplied matrices only; everything behind the generator tables
(the economised cos / sin pairs of the real loops, the core + border loop of D = 5, 9 and its fused tail, the schemes for normal
generators chosen from table flags, the real mid-D instance, the register-resident and tiled kernels on assembled generators,
every Lindblad path) is reached here.  One test = one case of tests/pwc_cases.py = one library call and one reference:

* the kernel instances of the call (`_lib.last_kernel_detail()`) are the recorded ones of the case's class
  (tests/golden/pwc_extended_kernels.json: launch logs of these very calls, as `tools/dispatch_table.py --probe` prints them);
* ||U_b - ref_b||_F <= 8 e_cpu for every sample, e_cpu the worst error over the samples of two double-precision CPU routes
  against the same reference: `oracle.propagate_batch`, and scipy's expm slice by slice under the oracle's fold.  8: the
  device polynomials may need up to three more squarings than Pade-13, and a squaring at most doubles the first-order bound
  (`CHAIN_FACTOR`, the 8 R_CPU of the expm bars).  Not tuned to what the kernels return;
* the same call again returns the same bits;
* with `want_dUs`, every slice's `expm_ratio` <= 8 x the worst ratio of scipy and the oracle over the same slices.

The scheme a case reaches is steered by the norm bound; tests/test_pwc_extended_ref.py asserts (without a GPU) that every case's
bound lies in the band it claims and that every slice stays inside the radius of Pade-13, which keeps e_cpu honest.
Every figure is printed before it is asserted (pytest -s shows the table DESIGN section 3 records).

Measured on one MI355X: 0.4 ... 7.3 x e_cpu everywhere except two classes, kept as strict expected failures (`OVER_THE_BAR`): the
small-D real loop with two squarings (12.3 ... 13.6) and the mid-D real instance with one squaring (8.66 ... 12.0).
"""
import json
import os

import numpy as np
import pytest

import extended_ref as x
import pwc_cases as pc

pytestmark = pytest.mark.gpu

_KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pwc_extended_kernels.json")
KERNELS = json.load(open(_KERNELS))


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def _call(prop, c, inp):
    from c3_amd import _lib

    with _lib.options(**dict(c.opts)):
        r = prop.propagate_batch(inp.h0, inp.hks, inp.signals, inp.dt, col_ops=inp.col, lindbladian=c.problem.lind is not None, fr_phase=inp.fr_phase, want_dUs=c.dUs)
        detail = _lib.last_kernel_detail()
    return np.asarray(r["U"]), (np.asarray(r["dUs"]) if c.dUs else None), detail


class BarExceeded(AssertionError):
    """The 8 e_cpu bar itself (an expected failure covers nothing else: kernel instance, shapes and repeatability still fail)."""


# Classes that EXCEED 8 e_cpu on the MI355X (e_device / e_cpu as measured; DESIGN section 3 has the per-slice breakdown).  The
# bar is not tuned to them: they stay expected failures until the maintainers decide, and a fix turns them into errors.
#  * small-D real loop, TWO squarings (norm bound in (3.7, 7.4]): every squaring doubles the error of the degree-8 pair, whose
#    truncation error (1.5e-16, about u by design) has the same sign in every slice and adds up over the chain;
#  * mid-D real instance, ONE squaring: cos 2Y = 2 C^2 - I quadruples the error of C where the small-D loop's (C - S)(C + S)
#    doubles it.
OVER_THE_BAR = {
    "sd-real-D5-K2-mm8+2": 13.6,
    "sd-real-D9-K2-mm8+2": 12.3,
    "sd-real-D9-above-3.7": 13.6,
    "md-real-D13-K3-mm8+1": 8.66,
    "md-real-D16-K4-mm8+1": 11.2,
    "md-real-D27-K3-mm8+1": 12.0,
    "md-real-D36-K4-mm8+1": 8.77,
}


def _param(c):
    if c.id not in OVER_THE_BAR:
        return pytest.param(c, id=c.id)
    reason = f"e_device / e_cpu = {OVER_THE_BAR[c.id]:g} measured on the MI355X (bar {x.CHAIN_FACTOR:g}): the scheme is less accurate than Pade-13 by more than the factor"
    return pytest.param(c, id=c.id, marks=pytest.mark.xfail(strict=True, raises=BarExceeded, reason=reason))


@pytest.mark.parametrize("c", [_param(c) for c in pc.CASES])
def test_pwc_against_extended_precision(prop, c):
    p = c.problem
    inp = pc.pwc_inputs(p)
    U, dUs, detail = _call(prop, c, inp)
    print(f"\nKERNEL {c.kernel} | {detail}")
    ref = pc.pwc_reference(p)
    Dm = p.D * p.D if p.lind else p.D
    assert U.shape == (p.B, Dm, Dm) and U.dtype == np.complex128
    e = x.pwc_err(U, ref.U)
    print(f"PWC {c.id} class={c.kernel} scheme={c.scheme} e_device={e:.3e} e_cpu={ref.e_cpu:.3e} (oracle {ref.e_oracle:.3e}, scipy {ref.e_scipy:.3e}) "
          f"e_device/e_cpu={e / ref.e_cpu:.3g} bar={x.CHAIN_FACTOR:g}")
    if dUs is not None:
        r = x.slices_ratio(dUs, ref.X, ref.dUs)
        print(f"PWC-SLICES {c.id} r_device={r:.3g} r_cpu={ref.r_cpu_slices:.3g} r_device/r_cpu={r / ref.r_cpu_slices:.3g} bar={x.EXPM_SLICE_FACTOR:g}")
    assert detail == KERNELS[c.kernel], (c.kernel, detail)
    # the same call again gives the same bits
    U2, dUs2, detail2 = _call(prop, c, inp)
    assert detail2 == detail
    assert x.same_bits(U, U2)
    if dUs is not None:
        assert x.same_bits(dUs, dUs2)
        x.check_pwc_slices(dUs, ref.X, ref.dUs, ref.r_cpu_slices)
    try:
        x.check_pwc(U, ref.U, ref.e_cpu)
    except AssertionError as err:
        raise BarExceeded(str(err)) from err
