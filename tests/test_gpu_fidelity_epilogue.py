"""GPU tests of the fidelity epilogue -- `overlap_kernel`, `infid_kernel`, `infid_sum_kernel` behind `c3p_gate_overlap` /
`c3p_gate_infid`, and the goal functions of `c3_amd.fidelities` built on them -- against extended precision
(tests/extended_ref.py), on both pointer routes.  Every optimiser's goal value passes through here.  -m gpu.

Bars, derived for ANY summation order (extended_ref.overlap_bar / infid_bar), T = sum |U_ac| |G_ac|:
    |s^ - s| <= delta_s = 2 (L^2 + 4) u T
    unitary   (2 |s| delta_s + delta_s^2) / L^2       + 4u
    average   (2 |s| delta_s + delta_s^2) / (L (L+1)) + 4u
    lindbladian  delta_t / L^2 + 4u,  delta_t over L^4 terms
    sum       sum_b bar_b + B u sum_b |f_b|
Shapes sit on the edges of the kernels: L^2 = 4 ... 1024 (tails next to exact multiples of the 64 lanes), B on both sides
of the 1024 samples one grid pass covers, unordered rows.  Out-of-range rows, wrong pointers or oversized counts are
never handed over on the device route: it is not validated.
"""
import ctypes

import numpy as np
import pytest

import extended_ref as x
from oracle import c3_oracle as o

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fid(lib):
    from c3_amd import fidelities, _lib

    _lib.require_gpu()
    return fidelities


# (dims, index) shapes through c3_amd.fidelities; L = 2^len(index)
FID_SHAPES = {
    "L2-D4": ([2, 2], [0]),
    "L4-D9": ([3, 3], [0, 1]),
    "L8-D27": ([3, 3, 3], [0, 1, 2]),
    "L16-D16": ([2, 2, 2, 2], [0, 1, 2, 3]),  # L^2 = 256: an exact multiple of 64
    "L32-D32": ([2] * 5, [0, 1, 2, 3, 4]),
}
# arbitrary row lists through the C ABI
ABI_SHAPES = {
    "abi-D9-L9": (9, list(range(9))),  # 81 = 64 + 17
    "abi-D9-rows8,0,4": (9, [8, 0, 4]),  # unordered
    "abi-D5-L1": (5, [2]),
}
B_EDGES = (1, 3, 4, 5, 1023, 1024, 1025, 2500)
INPUTS = ("unitary", "nonunitary", "ideal_block", "orthogonal_block")


def _batch_b(name):
    return B_EDGES if name in ("L2-D4", "L4-D9") else (1, 5)


def _unitaries(rng, B, D):
    q, r = np.linalg.qr(rng.normal(size=(B, D, D)) + 1j * rng.normal(size=(B, D, D)))
    d = np.diagonal(r, axis1=-2, axis2=-1)
    return q * (d / np.abs(d))[:, None, :]


def _inputs(kind, rng, B, D, rows, G):
    """U[B, D, D] of one input kind."""
    L = len(rows)
    ix = np.ix_(rows, rows)
    if kind == "unitary":
        return _unitaries(rng, B, D)
    Umat = np.broadcast_to(np.eye(D, dtype=np.complex128), (B, D, D)).copy()
    if kind == "ideal_block":  # the computational block EQUALS the ideal gate: infidelity 0 within the bar
        Umat[(slice(None),) + ix] = G
        return Umat
    if kind == "nonunitary":  # |s| > L (|s|^2 / L^2 ~ 1.44: the 4u of the epilogue's own roundings still holds)
        Umat[(slice(None),) + ix] = 1.2 * G
        return Umat + 0.02 * (rng.normal(size=(B, D, D)) + 1j * rng.normal(size=(B, D, D)))
    if kind == "orthogonal_block":  # s = tr(G V G^+) = tr V = 0: block G V, V = diag of the L-th roots of unity (L = 1: block 0)
        V = np.diag(np.exp(2j * np.pi * np.arange(L) / L)) if L > 1 else np.zeros((1, 1))
        Umat[(slice(None),) + ix] = G @ V
        return Umat
    raise ValueError(kind)


def _mixed(rng, B, D, rows, G):
    """Large batches: the four input kinds interleaved (sample b has kind b % 4)."""
    parts = [_inputs(k, rng, (B + 3) // 4, D, rows, G) for k in INPUTS]
    return np.ascontiguousarray(np.stack(parts, axis=1).reshape((-1, D, D))[:B])


class Abi:
    """c3p_gate_overlap / c3p_gate_infid on either pointer route, all arguments checked for size here (the device route
    of the library is not validated)."""

    def __init__(self, route):
        from c3_amd import _lib

        self.route, self.lib, self._lib = route, _lib.load(), _lib
        self.flags = _lib.HOST_PTRS if route == "host" else 0
        self.stream = None
        if route == "device":
            import torch

            self.torch = torch
            self.stream = torch.cuda.current_stream().cuda_stream

    def _in(self, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        return a if self.route == "host" else self.torch.as_tensor(a, device="cuda")

    def _out(self, n, dtype, fill):
        if self.route == "host":
            return np.full((n,), fill, dtype=dtype)
        return self.torch.full((n,), fill, dtype={np.float64: self.torch.float64, np.complex128: self.torch.complex128}[dtype], device="cuda")

    @staticmethod
    def _p(a):
        return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()

    def _done(self, *outs):
        if self.route == "device":
            self.torch.cuda.synchronize()
        return [x.to_np(t) for t in outs]

    def overlap(self, Umat, rows, G, B=None):
        B = Umat.shape[0] if B is None else B
        D, L = Umat.shape[-1], len(rows)
        assert Umat.shape == (max(B, 1), D, D) and G.shape == (L, L) and all(0 <= r < D for r in rows)
        u, r, g = self._in(Umat, np.complex128), self._in(rows, np.int32), self._in(G, np.complex128)
        out = self._out(max(B, 1), np.complex128, np.nan)
        rc = self.lib.c3p_gate_overlap(self._p(u), B, D, self._p(r), L, self._p(g), self.flags, self._p(out), self.stream)
        assert rc == 0, self.lib.c3p_last_error()
        return self._done(out)[0][:B]

    def infid(self, Umat, rows, G, kind, B=None):
        """(each[B], sum[2]); both buffers are pre-filled with NaN: every entry must be written."""
        B = Umat.shape[0] if B is None else B
        D, L = Umat.shape[-1], len(rows)
        assert Umat.shape == (max(B, 1), D, D) and G.shape == (L, L) and all(0 <= r < D for r in rows)
        u, r, g = self._in(Umat, np.complex128), self._in(rows, np.int32), self._in(G, np.complex128)
        each, tot = self._out(max(B, 1), np.float64, np.nan), self._out(2, np.float64, np.nan)
        rc = self.lib.c3p_gate_infid(self._p(u), B, D, self._p(r), L, self._p(g), {"unitary": 0, "average": 1}[kind], self.flags,
                                     self._p(each), self._p(tot), self.stream)
        assert rc == 0, self.lib.c3p_last_error()
        each, tot = self._done(each, tot)
        return each[:B], tot


def _check_epilogue(tag, route, Umat, rows, G, s_hat, unfused, each, tot):
    """The overlap, the unfused goal values, the fused ones and their sum against the long-double reference and each
    other; `unfused` / `each` / `tot` are dicts by kind."""
    B, L = Umat.shape[0], len(rows)
    r_s = x.check_overlap(s_hat, Umat, rows, G)
    s, T = x.overlap_ld(Umat, rows, G)
    line = [f"overlap {r_s:.3g}"]
    for kind in ("unitary", "average"):
        r_u = x.check_infid(unfused[kind], Umat, rows, G, kind)
        r_e = x.check_infid(each[kind], Umat, rows, G, kind)
        r_t = x.check_infid_sum(tot[kind][0], Umat, rows, G, kind)
        assert tot[kind][1] == float(B)
        assert np.all(np.abs(each[kind] - unfused[kind]) <= 2 * x.infid_bar(s, T, L, kind))
        line.append(f"{kind}: unfused {r_u:.3g} fused {r_e:.3g} sum {r_t:.3g}")
    print(f"FID {tag} B={B} {route}: error / bar  " + "  ".join(line))


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("name", list(FID_SHAPES))
def test_goal_functions_against_extended_precision(fid, name, route):
    dims, index = FID_SHAPES[name]
    rows = fid.computational_rows(dims, index)
    D, L = int(np.prod(dims)), len(rows)
    rng = np.random.default_rng([D, L])
    G = x.haar_unitary(rng, L)
    Gd = x.on_route(route, G)
    abi = Abi(route)
    for B in _batch_b(name):
        batches = {k: _inputs(k, rng, B, D, rows, G) for k in INPUTS} if B <= 5 else {"mixed": _mixed(rng, B, D, rows, G)}
        for kind_in, Umat in batches.items():
            Ud = x.on_route(route, Umat)
            s_hat, L_out = fid.gate_overlaps(Gd, Ud, index, dims)
            assert L_out == L
            unfused = {"unitary": x.to_np(fid.unitary_infid(Gd, Ud, index, dims)), "average": x.to_np(fid.average_infid(Gd, Ud, index, dims))}
            each, tot = {}, {}
            for kind in ("unitary", "average"):
                if B >= 1025:  # pre-filled with NaN: every entry written, the grid-stride loop leaves none out
                    each[kind], tot[kind] = abi.infid(Umat, rows, G, kind)
                else:
                    r = fid.infid_sum(Gd, Ud, index, dims, kind=kind, want_each=True)
                    each[kind], tot[kind] = x.to_np(r["each"]), x.to_np(r["sum"])
                    again = fid.infid_sum(Gd, Ud, index, dims, kind=kind, want_each=True)
                    assert x.same_bits(again["each"], each[kind]) and x.same_bits(again["sum"], tot[kind])
                only_sum = fid.infid_sum(Gd, Ud, index, dims, kind=kind)  # without the per-sample output
                assert only_sum["each"] is None and x.same_bits(only_sum["sum"], tot[kind])
            assert x.same_bits(fid.gate_overlaps(Gd, Ud, index, dims)[0], s_hat)
            _check_epilogue(f"{name} {kind_in}", route, Umat, rows, G, x.to_np(s_hat), unfused, each, tot)
            if kind_in == "ideal_block":  # no large negative value where the gate is perfect
                assert np.all(np.abs(each["unitary"]) <= 64 * L * L * x.U) and np.all(np.abs(unfused["average"]) <= 64 * L * L * x.U)
    # one matrix without a batch axis
    Umat = _inputs("unitary", rng, 1, D, rows, G)
    f1 = x.to_np(fid.unitary_infid(Gd, x.on_route(route, Umat[0]), index, dims))
    assert f1.shape == () and x.check_infid(f1, Umat[0], rows, G, "unitary") <= 1.0


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("name", list(ABI_SHAPES))
def test_abi_row_lists_against_extended_precision(lib, name, route):
    D, rows = ABI_SHAPES[name]
    L = len(rows)
    rng = np.random.default_rng([D, L, 7])
    G = x.haar_unitary(rng, L)
    abi = Abi(route)
    for B in (1, 5):
        for kind_in in INPUTS:
            Umat = _inputs(kind_in, rng, B, D, rows, G)
            s_hat = abi.overlap(Umat, rows, G)
            Lf = float(L)
            unfused = {"unitary": 1 - np.abs(s_hat / Lf) ** 2, "average": 1 - (np.abs(s_hat) ** 2 / Lf + 1) / (Lf + 1)}
            each, tot = {}, {}
            for kind in ("unitary", "average"):
                each[kind], tot[kind] = abi.infid(Umat, rows, G, kind)
                e2, t2 = abi.infid(Umat, rows, G, kind)
                assert x.same_bits(e2, each[kind]) and x.same_bits(t2, tot[kind])
            _check_epilogue(f"{name} {kind_in}", route, Umat, rows, G, s_hat, unfused, each, tot)


@pytest.mark.parametrize("route", x.ROUTES)
def test_empty_batch_sums_to_zero(lib, route):
    abi = Abi(route)
    rng = np.random.default_rng(5)
    G = x.haar_unitary(rng, 2)
    each, tot = abi.infid(_unitaries(rng, 1, 4), [0, 2], G, "unitary", B=0)
    assert each.shape == (0,) and tot.tolist() == [0.0, 0.0]
    assert abi.overlap(_unitaries(rng, 1, 4), [0, 2], G, B=0).shape == (0,)


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("dims", [[3, 3], [2, 2, 2]], ids=["81x81-16rows", "64x64-64rows"])
def test_lindbladian_route_against_extended_precision(fid, dims, route):
    """L^2 rows of a D^2 x D^2 superoperator: tf_super(U) times a weak (diagonal, contracting) dissipative map."""
    index = list(range(len(dims)))
    rows = fid.computational_rows(dims, index)
    D, L = int(np.prod(dims)), len(rows)
    srows = (rows[:, None].astype(np.int64) * D + rows[None, :]).reshape(-1)
    rng = np.random.default_rng([D, L, 3])
    G = x.haar_unitary(rng, L)
    Gs = x.kron_ld(G, np.conj(G))
    for B in (1, 5):
        for kind_in in ("unitary", "ideal_block"):
            Umat = _inputs(kind_in, rng, B, D, rows, G)
            damp = np.exp(-1e-3 * rng.uniform(0, 1, size=(B, 1, D * D)))
            S = np.ascontiguousarray(o.tf_super(Umat) * damp)
            Sd, Gd = x.on_route(route, S), x.on_route(route, G)
            f = x.to_np(fid.lindbladian_unitary_infid(Gd, Sd, index, dims))
            r = x.check_infid(f, S, srows, Gs, "lindbladian", L=L)
            assert x.same_bits(fid.lindbladian_unitary_infid(Gd, Sd, index, dims), f)
            print(f"FID lindbladian dims={dims} {kind_in} B={B} {route}: error / bar {r:.3g}")
            assert np.all(f > -64 * L**4 * x.U) and np.all(f < 1)
    f1 = x.to_np(fid.lindbladian_unitary_infid(Gd, x.on_route(route, S[0]), index, dims))
    assert f1.shape == () and x.check_infid(f1, S[0], srows, Gs, "lindbladian", L=L) <= 1.0


@pytest.mark.parametrize("route", x.ROUTES)
def test_refusals_are_return_codes(lib, route):
    """L > D, L = 0, an unknown kind -- and, on the host-pointer route only, a row outside [0, D): each is refused by the
    size checks of the entry point, before any launch.  All pointers are valid and all buffers large enough for the
    largest count handed over."""
    abi = Abi(route)
    rng = np.random.default_rng(9)
    D = 4
    u = abi._in(_unitaries(rng, 2, D), np.complex128)
    rows = abi._in(np.arange(D + 1) % D, np.int32)  # D + 1 valid entries
    g = abi._in(np.eye(D + 1), np.complex128)
    each, tot, ov = abi._out(2, np.float64, 0.0), abi._out(2, np.float64, 0.0), abi._out(2, np.complex128, 0.0)
    p = abi._p

    def infid(L, kind):
        return abi.lib.c3p_gate_infid(p(u), 2, D, p(rows), L, p(g), kind, abi.flags, p(each), p(tot), abi.stream)

    def overlap(L):
        return abi.lib.c3p_gate_overlap(p(u), 2, D, p(rows), L, p(g), abi.flags, p(ov), abi.stream)

    assert infid(D + 1, 0) != 0 and b"bad sizes" in abi.lib.c3p_last_error()
    assert infid(0, 0) != 0 and b"bad sizes" in abi.lib.c3p_last_error()
    assert infid(2, 2) != 0 and b"unknown infidelity kind" in abi.lib.c3p_last_error()
    assert overlap(D + 1) != 0 and overlap(0) != 0
    if route == "host":
        for bad in (D, -1):
            r = np.array([0, bad], dtype=np.int32)
            assert abi.lib.c3p_gate_infid(p(u), 2, D, r.ctypes.data, 2, p(g), 0, abi.flags, p(each), p(tot), None) != 0
            assert b"outside [0,4)" in abi.lib.c3p_last_error()
            assert abi.lib.c3p_gate_overlap(p(u), 2, D, r.ctypes.data, 2, p(g), abi.flags, p(ov), None) != 0
    # the entry points work afterwards
    assert infid(2, 0) == 0 and overlap(2) == 0


def test_goal_function_refusals(fid):
    from c3_amd._lib import C3PropError

    Umat = np.eye(4, dtype=np.complex128)[None]
    G = np.eye(2, dtype=np.complex128)
    with pytest.raises(C3PropError, match="unknown infidelity kind"):
        fid.infid_sum(G, Umat, [0], [2, 2], kind="state")
    with pytest.raises(C3PropError, match="do not match"):
        fid.infid_sum(G, Umat, [0], [3, 3])
    with pytest.raises(C3PropError, match=r"must be \[2,2\]"):
        fid.gate_overlaps(np.eye(4, dtype=np.complex128), Umat, [0], [2, 2])
