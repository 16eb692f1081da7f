"""Host side of the small-D model record: the size mirror against the library, and the numpy restatement of the tables that the
GPU test (tests/test_gpu_smalld_model_record.py) reads the device's record against.  No GPU."""
import numpy as np

from c3_amd import _record


def test_record_bytes_mirror_matches_the_library(lib):
    for D in range(1, 17):
        for K in range(0, 5):
            want = int(lib.c3p_pwc_record_bytes(D, K))
            assert _record.record_bytes(D, K) == want, (D, K)
            assert (want == 0) == (D < 2 or D > 12), (D, K)
    assert lib.c3p_pwc_record_bytes(9, -1) == 0 and _record.record_bytes(9, -1) == 0
    assert lib.c3p_pwc_record_bytes(9, 9) == 0 and _record.record_bytes(9, 9) == 0  # the small-D route takes K <= 8
    # cfg2: three tables of 5 x 4 rows of 13 doubles + 4 words, and 16 column sums each
    assert _record.record_bytes(9, 2) == 8 * 3 * (260 + 4 + 16)


def test_build_without_a_served_shape_is_an_error(lib):
    assert lib.c3p_pwc_record_build(None, None, 1.0, 2, 13, 0, None, None) != 0
    assert b"no record is served" in lib.c3p_last_error()


def test_reference_tables_restate_the_generators():
    rng = np.random.default_rng(21)
    D, K, dt = 5, 2, 0.37
    h = rng.normal(size=(1 + K, D, D)) + 1j * rng.normal(size=(1 + K, D, D))
    G, mu, cs = _record.reference_tables(h[0], h[1:], dt)
    for k in range(1 + K):
        g = -1j * dt * h[k]
        m = np.trace(g).imag / D
        want = g - 1j * m * np.eye(D)
        assert np.allclose(G[k], want, rtol=0, atol=1e-15)
        assert abs(np.trace(G[k]).imag) < 1e-14 and np.isclose(np.trace(G[k]).real, np.trace(g).real)  # imaginary shift only
        assert np.isclose(mu[k], m)
        assert np.allclose(cs[k], np.abs(want).sum(axis=0))
    # a real symmetric Hamiltonian: a purely imaginary generator
    hs = rng.normal(size=(D, D))
    G, _, _ = _record.reference_tables(hs + hs.T, np.zeros((0, D, D)), dt)
    assert G.shape == (1, D, D) and not G.real.any()


def test_unpack_reads_the_half_image_layout():
    D, K = 3, 1
    MAT, W = _record.mat_doubles(D), _record.row_stride(D)
    assert (MAT, W) == (4 * 2 * 5, 5)
    rng = np.random.default_rng(22)
    G = rng.normal(size=(1 + K, D, D)) + 1j * rng.normal(size=(1 + K, D, D))
    rec = np.zeros(_record.record_bytes(D, K) // 8)
    for k in range(1 + K):
        t = rec[k * (MAT + 4) : (k + 1) * (MAT + 4)]
        for i in range(D):
            t[(2 * i) * W : (2 * i) * W + D] = G[k, i].real
            t[(2 * i + 1) * W : (2 * i + 1) * W + D] = G[k, i].imag
        t[MAT : MAT + 4] = [0.0, 0.5 + k, 2.0 + k, -3.0 * k]
    T = (1 + K) * (MAT + 4)
    rec[T:] = np.arange(16 * (1 + K))
    got = _record.unpack_record(rec, D, K)
    assert np.array_equal(got["G"], G) and not got["padding"].any()
    assert np.array_equal(got["mu"], [[0.0, 0.5], [0.0, 1.5]]) and np.array_equal(got["norm1"], [2.0, 3.0]) and np.array_equal(got["flag"], [0.0, -3.0])
    assert np.array_equal(got["colsums"], np.arange(32.0).reshape(2, 16))
    rec[W - 1] = 1.0  # a word of the padding column
    assert _record.unpack_record(rec, D, K)["padding"].any()
    try:
        _record.unpack_record(rec[:-1], D, K)
        raise AssertionError("a short record was accepted")
    except ValueError:
        pass
