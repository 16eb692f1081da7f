"""GPU tests of the matrix routines everything else is built from -- `propagation.expm`, `tf_matmul_left/right/n`,
`tf_kron`, `tf_spre`, `tf_spost`, `tf_super` -- against extended precision (tests/extended_ref.py), at every kernel class
and plan edge, on both pointer routes (numpy in: host pointers; CUDA tensors in: device pointers).  -m gpu.

Bars (none of them tuned to what the kernels return):
* expm: r = ||E - E_ref||_max / (u max(1, ||A||_1) ||E_ref||_max) <= 8 R_CPU_EXPM[class], R_CPU_EXPM the worst of scipy and
  the oracle over the same matrices (tests/test_extended_ref.py).  8: the device polynomial (radius 1.13) needs up to
  ceil(log2(5.37 / 1.13)) = 3 more squarings than Pade-13, and a squaring at most doubles the first-order bound;
* chains: error <= 8 x the error of the oracle's double-precision fold of the same factors;
* tf_kron / tf_super: one rounded complex product per entry (4u |a||b|); tf_spre / tf_spost: bit-exact.
Every ratio is printed before it is asserted (pytest -s shows the table DESIGN section 3 records).
"""
import numpy as np
import pytest

import extended_ref as x

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prop(lib):
    from c3_amd import propagation, _lib

    _lib.require_gpu()
    return propagation


def _expected_kernel(D: int, force_generic: bool = False) -> str:
    if force_generic or D < 2 or D > 40:
        return "generic_lds" if D <= 37 else "generic_global"
    return "smalld" if D <= 12 else "mfma"


# --------------------------------------------------------------------------
# expm
# --------------------------------------------------------------------------

EXPM_CASES = x.expm_cases()


def _expm_in_chunks(prop, c, A, route):
    from c3_amd import _lib

    out = []
    for i in range(0, A.shape[0], c.chunk):
        out.append(x.to_np(prop.expm(x.on_route(route, A[i : i + c.chunk]), force_generic=c.force_generic)))
        assert _lib.last_kernel() == _expected_kernel(c.D, c.force_generic), (x.case_id(c), _lib.last_kernel())
    return np.concatenate(out)


def _check_expm_case(prop, c, route, tag):
    A, E_ref = x.expm_inputs(c)
    E = _expm_in_chunks(prop, c, A, route)
    assert E.shape == A.shape and E.dtype == np.complex128
    worst = {}
    for i in range(A.shape[0]):
        k = x.expm_class(c, A[i])
        r = x.expm_ratio(E[i], A[i], E_ref[i])
        if c.kind == "skewherm":
            r = max(r, x.unitarity_ratio(E[i], A[i]))  # E^+ E = 1 within the bar of the error itself
        if r > worst.get(k, (-1.0, 0))[0]:
            worst[k] = (r, i)
    for k, (r, i) in sorted(worst.items()):
        print(f"{tag} {x.case_id(c)} {route} class={k} r_device={r:.4g} bar={x.class_bar(k):.4g} at matrix {i} (norm {x.norm1(A[i]):.4g})")
    for k, (r, i) in worst.items():
        assert r <= x.class_bar(k), (x.case_id(c), route, k, r, i, x.device_norm(A[i]))
    # the same call again gives the same bits
    assert x.same_bits(E, _expm_in_chunks(prop, c, A, route))
    # exp(0) = 1 bit for bit
    for i in range(A.shape[0]):
        if not A[i].any():
            assert x.same_bits(E[i], np.eye(c.D, dtype=np.complex128)), (x.case_id(c), i)


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("c", EXPM_CASES, ids=[x.case_id(c) for c in EXPM_CASES])
def test_expm_against_extended_precision(prop, c, route):
    _check_expm_case(prop, c, route, "EXPM")


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("c", x.EXPM_MIXED_CASES, ids=[x.case_id(c) for c in x.EXPM_MIXED_CASES])
def test_expm_small_norm_next_to_large_norm(prop, c, route):
    """Two matrices of norm 1e-9 in one call with two of norm 40, each held to the bar of its own class.

    The small-D kernel runs four matrices per wave and takes the polynomial and its loop counts wave-uniformly from the
    LARGEST of their norms.  Until this test existed it took scaling and squarings from there too: next to a norm of 40
    (six squarings) the matrix of norm 1e-9 was computed as (1 + X / 64)^64, every squaring doubling the rounding error of
    the ones on its diagonal -- r = 104.9 against a bar of 47.2 at D = 9 (1.5e-14 absolute, but exp(A) - 1 kept five
    digits), and 48.8 / 132.8 / 87.0 at D = 3 / 9 / 12 over batches of 260 matrices in arbitrary order of norm, where one
    matrix per call stayed below 14.  Now every chain scales by its own norm and keeps its result through the squarings it
    does not need (c3p_smalld.hip, supplied-generator mode): r = 1.9.  The mid-D and generic kernels plan per matrix."""
    _check_expm_case(prop, c, route, "EXPM-MIXED")


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("D", [1, 2, 3, 9, 12, 13, 27, 40, 41, 64])
def test_expm_of_zero_is_the_identity_bit_for_bit(prop, D, route):
    E = x.to_np(prop.expm(x.on_route(route, np.zeros((3, D, D), dtype=np.complex128))))
    assert x.same_bits(E, np.broadcast_to(np.eye(D, dtype=np.complex128), (3, D, D)))


@pytest.mark.parametrize("route", x.ROUTES)
def test_expm_size_limits(prop, route):
    """n = 0 returns an empty array; D = 257 is refused by the size check of the generic kernel (D <= 256), before any
    launch."""
    from c3_amd._lib import C3PropError

    E = x.to_np(prop.expm(x.on_route(route, np.zeros((0, 5, 5), dtype=np.complex128))))
    assert E.shape == (0, 5, 5)
    with pytest.raises(C3PropError, match="exceeds the generic kernel limit"):
        prop.expm(x.on_route(route, np.zeros((1, 257, 257), dtype=np.complex128)))
    # the library is usable afterwards
    E = x.to_np(prop.expm(x.on_route(route, np.zeros((2, 2), dtype=np.complex128))))
    assert x.same_bits(E, np.eye(2, dtype=np.complex128))


# --------------------------------------------------------------------------
# ordered products
# --------------------------------------------------------------------------


def _chain_checks(prop, ref, route, D, label):
    """left, right, tf_matmul_n and left again (the workspace slots of the first call are reused in between)."""
    from c3_amd import _lib

    kernel = _expected_kernel(D)
    M = x.on_route(route, ref.M)
    out = {}
    for name, fn in (("left", prop.tf_matmul_left), ("right", prop.tf_matmul_right), ("n", prop.tf_matmul_n), ("left2", prop.tf_matmul_left)):
        out[name] = x.to_np(fn(M))
        assert _lib.last_kernel() == kernel, (label, name, _lib.last_kernel())
        assert out[name].shape == ref.left.shape
    r_l = x.check_chain(out["left"], ref.left, ref.e_left)
    r_r = x.check_chain(out["right"], ref.right, ref.e_right)
    r_n = x.check_chain(out["n"], ref.left, ref.e_left)
    print(f"CHAIN {label} {route} e_device/e_cpu left={r_l:.3g} right={r_r:.3g} n={r_n:.3g} (e_cpu {ref.e_left:.3g} / {ref.e_right:.3g})")
    assert x.same_bits(out["left"], out["left2"]) and x.same_bits(out["left"], out["n"])
    return out


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("D", x.CHAIN_DIMS)
def test_chain_against_extended_precision(prop, D, route):
    """Every fold edge of the kernel family of D (extended_ref.CHAIN_N_*), B = 1 and 5, 4-D input and (B = 1) 3-D input.
    N = 1 (e_cpu = 0) must return its input bit for bit: the chain kernels start from the first factor, not from an identity
    they would have to multiply by."""
    for N in x.chain_lengths(D):
        for B in x.chain_batches(D, N):
            ref = x.chain_inputs(D, N, B)
            out = _chain_checks(prop, ref, route, D, f"D{D}-N{N}-B{B}")
            if N == 1:
                assert x.same_bits(out["left"], ref.M[:, 0]) and x.same_bits(out["right"], ref.M[:, 0])
            if B == 1:  # 3-D input: squeezed result, same bits
                M3 = x.on_route(route, ref.M[0])
                l3, r3 = x.to_np(prop.tf_matmul_left(M3)), x.to_np(prop.tf_matmul_right(M3))
                assert l3.shape == (D, D)
                assert x.same_bits(l3, out["left"][0]) and x.same_bits(r3, out["right"][0])


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("D,N", [(9, 33), (27, 33), (41, 17)])
def test_chain_of_general_factors(prop, D, N, route):
    """General complex N(0,1)/sqrt(D) factors (no structure a unitary-only mistake could hide behind), one case per kernel."""
    _chain_checks(prop, x.chain_inputs(D, N, 5, True), route, D, f"general-D{D}-N{N}-B5")


@pytest.mark.parametrize("route", x.ROUTES)
def test_chain_refusals(prop, route):
    from c3_amd._lib import C3PropError

    with pytest.raises(C3PropError, match="exceeds the generic kernel limit"):
        prop.tf_matmul_left(x.on_route(route, np.zeros((1, 2, 257, 257), dtype=np.complex128)))


# --------------------------------------------------------------------------
# kron / spre / spost / super
# --------------------------------------------------------------------------

KRON_CASES = [((1, 1), (1,)), ((1, 1), (3,)), ((2, 3), (1,)), ((2, 3), (3,)), ((2, 3), (1000,)), ((2, 3), (2, 3)), ((3, 2), (1,)), ((3, 2), (3,)),
              ((1, 7), (3,)), ((16, 5), (1,)), ((16, 5), (3,)), ((9, 9), (1,)), ((9, 9), (3,)), ((27, 27), (1,))]


def _kron_inputs(Da, Db, batch):
    """Complex, non-symmetric, non-Hermitian, no two entries alike."""
    rng = np.random.default_rng([Da, Db, len(batch), batch[0]])
    A = rng.normal(size=batch + (Da, Da)) + 1j * rng.normal(size=batch + (Da, Da))
    B = rng.normal(size=batch + (Db, Db)) + 1j * rng.normal(size=batch + (Db, Db))
    return A, B


@pytest.mark.parametrize("route", x.ROUTES)
@pytest.mark.parametrize("dims,batch", KRON_CASES, ids=[f"{a}x{b}-n{'x'.join(map(str, n))}" for (a, b), n in KRON_CASES])
def test_kron_and_superoperators(prop, dims, batch, route):
    Da, Db = dims
    A, B = _kron_inputs(Da, Db, batch)
    K = x.to_np(prop.tf_kron(x.on_route(route, A), x.on_route(route, B)))
    r_k = x.check_kron(K, A, B)
    assert x.same_bits(K, prop.tf_kron(x.on_route(route, A), x.on_route(route, B)))
    r_s = 0.0
    for M in (A, B) if Da != Db else (A,):
        Md = x.on_route(route, M)
        x.check_exact(x.to_np(prop.tf_spre(Md)), x.spre_ref(M))
        x.check_exact(x.to_np(prop.tf_spost(Md)), x.spost_ref(M))
        S = x.to_np(prop.tf_super(Md))
        r_s = max(r_s, x.check_kron(S, M, np.conj(M)))  # A (x) conj(A): neither A (x) A nor A (x) A^+
        assert x.same_bits(S, prop.tf_super(Md))
    print(f"KRON {dims} n={batch} {route}: worst |err| / (4u|a||b|) kron={r_k:.3g} super={r_s:.3g}; spre / spost bit-exact")


@pytest.mark.parametrize("route", x.ROUTES)
def test_kron_refuses_mismatched_batches(prop, route):
    from c3_amd._lib import C3PropError

    A, B = _kron_inputs(2, 3, (3,))
    with pytest.raises(C3PropError, match="equal batch shapes"):
        prop.tf_kron(x.on_route(route, A), x.on_route(route, B[:2]))
    with pytest.raises(C3PropError, match="equal batch shapes"):
        prop.tf_kron(x.on_route(route, A[0]), x.on_route(route, B))
