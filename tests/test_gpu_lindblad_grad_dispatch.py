"""Dispatch of the open-system gradient entry points, pinned: which kernels every call launches, in which order and how often.

For a grid of small calls made through c3_amd.propagation the pair (_lib.last_kernel(), _lib.last_kernel_detail()) is compared,
as strings, with tests/golden/lindblad_grad_dispatch.json.  The golden is the library's own launch log, recorded with

    python tests/test_gpu_lindblad_grad_dispatch.py --record

on the commit before the host layer of these entry points was consolidated: a change of that layer that moves a call to another
kernel family, reorders its launches, changes a template argument or the number of sample chunks shows up here.  Results are
not checked here (tests/test_gradient.py, tests/test_gpu_round4.py, tests/test_gpu_lindblad_model_grad*.py do that).

The grid (CASES): c3p_pwc_lindblad_vjp at D = 2 .. 9, the model-cotangent entries (D = 2 .. 6 general, D = 7, 8, 9 in the Hermitian
basis), the taped pair (forward call and tape.vjp: two records), and the supplied-generator gradient of propagate_per_slice_vjp at
one small-D and one mid-D size; Hermitian and non-Hermitian Hamiltonians at D = 2, 3, 4, 7, shared and per-sample collapse
operators, the options that move the dispatch at one shape each, and grad_chunk = 2 on B = 5 (three chunks: the xN counts).
A call the library refuses is recorded by its error text.  Shapes: B = 3, K = 2, C = 1, N = 24 (D <= 6) or 16 (D >= 7)."""
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the recorder is run as a script: the package is one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from c3_amd import _lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lindblad_grad_dispatch.json")
DT, K, C = 0.3, 2, 1


def _case(entry, D, herm=True, col_ps=False, h0_ps=False, B=3, **opts):
    name = f"{entry}-D{D}-{'herm' if herm else 'nonherm'}" + ("-colps" if col_ps else "") + ("-h0ps" if h0_ps else "")
    name += "".join(f"-{k}={v}" for k, v in sorted(opts.items())) + (f"-B{B}" if B != 3 else "")
    return {"name": name, "entry": entry, "D": D, "herm": herm, "col_ps": col_ps, "h0_ps": h0_ps, "B": B, "opts": opts}


def _cases():
    c = []
    for D in range(2, 10):
        c.append(_case("vjp", D))
    for D in range(2, 7):
        c.append(_case("model", D))
    for D in (7, 8, 9):
        c.append(_case("hb", D))
    for D in (2, 3, 4, 7, 8, 9):
        c.append(_case("taped", D))
    for D in (2, 3, 4, 7):
        c.append(_case("vjp", D, herm=False))
        c.append(_case("taped", D, herm=False))
    for D in (2, 3, 4):
        c.append(_case("model", D, herm=False))
    c.append(_case("hb", 7, herm=False))
    for D in (3, 4, 5, 7):
        c.append(_case("vjp", D, col_ps=True))
    c.append(_case("vjp", 3, herm=False, col_ps=True))
    c.append(_case("model", 3, col_ps=True))
    c.append(_case("hb", 7, col_ps=True))
    c.append(_case("vjp", 3, h0_ps=True))
    c.append(_case("taped", 3, h0_ps=True))
    c.append(_case("taped", 3, herm=False, h0_ps=True))
    c.append(_case("xg", 3))
    c.append(_case("xg", 16))
    c.append(_case("vjp", 3, valu_grad=1))
    c.append(_case("vjp", 5, valu_grad=1))
    c.append(_case("vjp", 3, tiled_grad=1))
    c.append(_case("vjp", 3, no_smallr=1))
    c.append(_case("vjp", 4, no_smallr=1))
    c.append(_case("taped", 3, no_smallr=1))
    c.append(_case("vjp", 7, no_hermitian_basis=1))
    c.append(_case("vjp", 6, regr_grad_d6=1))
    c.append(_case("hb", 6, regr_grad_d6=1))
    for entry, D in (("vjp", 3), ("vjp", 4), ("vjp", 5), ("vjp", 7), ("model", 3), ("hb", 7), ("xg", 3), ("xg", 16)):
        c.append(_case(entry, D, B=5, grad_chunk=2))
    c.append(_case("vjp", 3, herm=False, B=5, grad_chunk=2))
    return c


CASES = _cases()


def inputs(case):
    """seeded operators, controls and cotangent of one case, as numpy arrays"""
    D, B = case["D"], case["B"]
    N = 24 if D <= 6 else 16
    rng = np.random.default_rng(9100 + 10 * D + B)
    g = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    herm = lambda a: (a + np.conj(np.swapaxes(a, -1, -2))) / 2
    if case["entry"] == "xg":
        return {"hs": herm(g(B, N, D, D)), "U_bar": g(B, D, D), "N": N}
    h0 = 0.8 * herm(g(B, D, D) if case["h0_ps"] else g(D, D))
    hks = 0.5 * herm(g(K, D, D))
    if not case["herm"]:
        h0, hks = h0 + 0.1 * g(*h0.shape), hks + 0.1 * g(*hks.shape)
    col = 0.2 * (g(B, C, D, D) if case["col_ps"] else g(C, D, D))
    return {"h0": h0, "hks": hks, "col": col, "sig": rng.uniform(-1, 1, size=(B, K, N)), "U_bar": g(B, D * D, D * D), "N": N}


def run_case(prop, case):
    """-> (records [[last_kernel, last_kernel_detail], ...], outputs {name: tensor}) of one case; a refused call is recorded as
    ["error", <the message>]"""
    import torch

    x = {k: torch.as_tensor(v, device="cuda:0") for k, v in inputs(case).items() if k != "N"}
    note = lambda: [_lib.last_kernel(), _lib.last_kernel_detail()]
    recs, out = [], {}
    with _lib.options(**case["opts"]):
        try:
            if case["entry"] == "xg":
                out["Z"] = prop.propagate_per_slice_vjp(x["hs"], DT, x["U_bar"])
                recs.append(note())
            elif case["entry"] == "taped":
                r = prop.propagate_batch_lindblad_taped(x["h0"], x["hks"], x["sig"], DT, x["col"])
                recs.append(note())
                out["U"] = r["U"]
                out["grad_signals"] = r["tape"].vjp(x["U_bar"])
                recs.append(note())
            else:
                kw = {"vjp": {}, "model": {"want_model_grads": True}, "hb": {"want_model_grads": True, "hermitian_basis": True}}[case["entry"]]
                r = prop.propagate_batch_lindblad_vjp(x["h0"], x["hks"], x["sig"], DT, x["col"], x["U_bar"], **kw)
                recs.append(note())
                r = r if isinstance(r, tuple) else (r,)
                out.update(zip(("grad_signals", "grad_h0", "grad_hks", "grad_col_ops"), r))
        except _lib.C3PropError as e:
            recs.append(["error", str(e)])
    torch.cuda.synchronize()
    return recs, out


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation

    _lib.require_gpu()
    return propagation


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_grid_and_golden_agree(golden):
    assert sorted(golden) == sorted(c["name"] for c in CASES)
    assert len(golden) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dispatch_is_pinned(prop, golden, case):
    recs, _ = run_case(prop, case)
    for got, want in zip(recs, golden[case["name"]]):
        print(case["name"], got)
        assert got == want
    assert len(recs) == len(golden[case["name"]])


if __name__ == "__main__":
    from c3_amd import propagation

    assert sys.argv[1:] == ["--record"], __doc__
    _lib.require_gpu()
    table = {c["name"]: run_case(propagation, c)[0] for c in CASES}
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(table)} cases -> {GOLDEN}")
