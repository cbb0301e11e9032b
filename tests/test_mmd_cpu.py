"""tuplewise.mmd without a GPU: the NumPy oracle the GPU tests compare against (distances by the
oracle of tests/test_triplets_cpu.py, components by math.fsum over the terms, the estimators
restated literally with the same np.random calls in the same order), the oracle against a
brute-force double loop and against the textbook definitions, every argument error before any
device work or RNG draw, and the native entry points' argument checks."""
import ctypes
import math

import numpy as np
import pytest

from test_triplets_cpu import data, o_dist_pairs, o_dist_rows, same_state

KERNELS = ["gaussian", "energy"]


# ------------------------------------------------------------------------------------ oracle
def o_coef(kernel, sigma):
    return -1.0 / (2.0 * sigma * sigma) if kernel == "gaussian" else None


def o_g(D, kernel, sigma):
    """g of an array of squared distances: np.exp(D * c) or np.sqrt(D)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(D * o_coef(kernel, sigma)) if kernel == "gaussian" else np.sqrt(D)


def o_fsum(terms):
    """math.fsum of the terms, NaN if any term is NaN (fsum raises on inf - inf only)."""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    if np.isnan(terms).any():
        return float("nan")
    return math.fsum(terms.tolist())


def o_components(X, Z, kernel, sigma=None):
    """(Sxx, Szz, Sxz): the sums over i < j, k < l and all (i, k)."""
    n, m = len(X), len(Z)
    gxx, gzz = o_g(o_dist_rows(X, X), kernel, sigma), o_g(o_dist_rows(Z, Z), kernel, sigma)
    gxz = o_g(o_dist_rows(X, Z), kernel, sigma)
    return (o_fsum(gxx[np.triu_indices(n, 1)]), o_fsum(gzz[np.triu_indices(m, 1)]), o_fsum(gxz))


def o_parts(X, Z, kernel, sigma=None):
    """The three terms of V: 2 Sxx / (n (n - 1)), 2 Szz / (m (m - 1)), 2 Sxz / (n m)."""
    n, m = len(X), len(Z)
    sxx, szz, sxz = o_components(X, Z, kernel, sigma)
    return 2.0 * sxx / (n * (n - 1)), 2.0 * szz / (m * (m - 1)), 2.0 * sxz / (n * m)


def o_sign(kernel):
    return 1.0 if kernel == "gaussian" else -1.0


def o_Un(X, Z, kernel, sigma=None):
    a, b, c = o_parts(X, Z, kernel, sigma)
    return np.float64(o_sign(kernel) * (a + b - c))


def o_Un_scale(X, Z, kernel, sigma=None):
    """The magnitude the statistic's tolerance is taken from: the sum of |terms| of V."""
    return sum(abs(t) for t in o_parts(X, Z, kernel, sigma))


def o_idx_sums(X, Z, i, j, k, l, kernel, sigma=None):  # noqa: E741
    """(s0, s1, s2, s3) = sums of g(x_i, x_j), g(z_k, z_l), g(x_i, z_l), g(x_j, z_k)."""
    X, Z = X.reshape(len(X), -1), Z.reshape(len(Z), -1)
    return tuple(o_fsum(o_g(o_dist_pairs(A, B), kernel, sigma))
                 for A, B in ((X[i], X[j]), (Z[k], Z[l]), (X[i], Z[l]), (X[j], Z[k])))


def o_UB_indices(X, Z, i, j, k, l, kernel, sigma=None):  # noqa: E741
    if len(i) == 0:
        return np.float64("nan")
    s = o_idx_sums(X, Z, i, j, k, l, kernel, sigma)
    return np.float64(o_sign(kernel) * (s[0] + s[1] - s[2] - s[3]) / len(i))


def o_UB_scale(X, Z, i, j, k, l, kernel, sigma=None):  # noqa: E741
    return sum(o_idx_sums(X, Z, i, j, k, l, kernel, sigma)) / len(i)


def o_draw(n, m, B):
    i = np.random.randint(0, n, B)
    j = np.random.randint(0, n - 1, B)
    j += (j >= i)
    k = np.random.randint(0, m, B)
    l = np.random.randint(0, m - 1, B)  # noqa: E741
    l += (l >= k)  # noqa: E741
    return i, j, k, l


def o_UB(X, Z, B, kernel, sigma=None):
    i, j, k, l = o_draw(X.shape[0], Z.shape[0], B)  # noqa: E741
    return o_UB_indices(X, Z, i, j, k, l, kernel, sigma)


def o_UN(X, Z, N, f_block):
    np.random.shuffle(X)
    np.random.shuffle(Z)
    k, kz = int(X.shape[0] / N), int(Z.shape[0] / N)
    return np.mean([f_block(X[b * k:(b + 1) * k], Z[b * kz:(b + 1) * kz]) for b in range(N)])


def o_UnN(X, Z, N, kernel, sigma=None):
    return o_UN(X, Z, N, lambda x, z: o_Un(x, z, kernel, sigma))


def o_UnNB(X, Z, N, B, kernel, sigma=None):
    return o_UN(X, Z, N, lambda x, z: o_UB(x, z, B, kernel, sigma))


def o_UnNT(X, Z, N, T, kernel, sigma=None):
    return np.mean([o_UnN(X, Z, N, kernel, sigma) for _ in range(T)])


def o_UnNBT(X, Z, N, B, T, kernel, sigma=None):
    return np.mean([o_UnNB(X, Z, N, B, kernel, sigma) for _ in range(T)])


# ------------------------------------------------------------------- the oracle's own checks
def brute_g(a, b, kernel, sigma):
    """g by the definition: Python floats, ascending coordinates."""
    acc = 0.0
    for c in range(len(a)):
        t = float(a[c]) - float(b[c])
        acc = acc + t * t
    if kernel == "gaussian":
        return math.exp(acc * (-1.0 / (2.0 * sigma * sigma)))
    return math.sqrt(acc)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,m,d", [(2, 2, 1), (7, 5, 3), (6, 7, 17)])
def test_oracle_is_the_double_loop(kernel, n, m, d):
    X, Z = data("gauss", n, m, d, 3)
    sigma = math.sqrt(d) if kernel == "gaussian" else None
    sxx = math.fsum(brute_g(X[i], X[j], kernel, sigma) for i in range(n) for j in range(i + 1, n))
    szz = math.fsum(brute_g(Z[k], Z[l], kernel, sigma) for k in range(m) for l in range(k + 1, m))
    sxz = math.fsum(brute_g(X[i], Z[k], kernel, sigma) for i in range(n) for k in range(m))
    got = o_components(X, Z, kernel, sigma)
    # math.exp and np.exp may differ in the last bit of a term; sqrt is exact on both sides
    assert np.allclose(got, (sxx, szz, sxz), rtol=1e-14 if kernel == "gaussian" else 0, atol=0)


def test_oracle_gaussian_is_the_textbook_mmd():
    X, Z = data("gauss", 23, 17, 4, 5)
    sigma = 1.7
    n, m = len(X), len(Z)

    def gram(A, B):
        sq = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
        return np.exp(-sq / (2 * sigma ** 2))

    Kxx, Kzz, Kxz = gram(X, X), gram(Z, Z), gram(X, Z)
    want = ((Kxx.sum() - np.trace(Kxx)) / (n * (n - 1)) + (Kzz.sum() - np.trace(Kzz)) / (m * (m - 1))
            - 2.0 * Kxz.mean())
    assert abs(o_Un(X, Z, "gaussian", sigma) - want) <= 1e-13


def test_oracle_energy_is_the_energy_distance():
    X, Z = data("gauss", 19, 26, 3, 6)

    def mean_norm(A, B, off_diagonal):
        D = np.linalg.norm(A[:, None, :] - B[None, :, :], axis=-1)
        return D.sum() / (len(A) * (len(A) - 1)) if off_diagonal else D.mean()

    want = 2.0 * mean_norm(X, Z, False) - mean_norm(X, X, True) - mean_norm(Z, Z, True)
    assert abs(o_Un(X, Z, "energy") - want) <= 1e-12 * (2.0 * mean_norm(X, Z, False))


@pytest.mark.parametrize("kernel", KERNELS)
def test_oracle_is_the_mean_of_h_over_quadruples(kernel):
    n = m = 5
    X, Z = data("gauss", n, m, 3, 7)
    sigma = 1.3 if kernel == "gaussian" else None
    i, j, k, l = (a.reshape(-1) for a in np.meshgrid(*[np.arange(5)] * 4, indexing="ij"))  # noqa: E741
    keep = (i != j) & (k != l)
    got = o_UB_indices(X, Z, i[keep], j[keep], k[keep], l[keep], kernel, sigma)
    assert abs(got - o_Un(X, Z, kernel, sigma)) <= 1e-12 * o_Un_scale(X, Z, kernel, sigma)


def test_oracle_nan_and_ties():
    X, Z = data("nan", 9, 6, 4, 8)  # one NaN coordinate in X: Sxx and Sxz are NaN, Szz is not
    sxx, szz, sxz = o_components(X, Z, "energy")
    assert np.isnan(sxx) and np.isnan(sxz) and not np.isnan(szz)
    X2 = np.ones((2, 3))
    assert o_components(X2, X2, "gaussian", 1.0)[0] == 1.0
    assert o_components(X2, X2, "energy")[0] == 0.0


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.mmd as mm
    for name in ("components", "Un", "UB_indices", "UB", "UN", "UnN", "UnNB", "UnNT", "UnNBT"):
        assert callable(getattr(mm, name)), name
    assert mm.MAX_D == 64


def test_argument_errors_need_no_device(tw):
    import tuplewise.mmd as mm
    X, Z = np.arange(40.0).reshape(10, 4), np.arange(24.0).reshape(6, 4) + 0.5
    X0, Z0 = X.copy(), Z.copy()
    x1 = np.arange(10.0)
    wide = np.zeros((4, 65))
    E = dict(kernel="energy")
    G = dict(sigma=1.0)
    state = np.random.get_state()
    calls = [
        # dtype, layout, rank
        lambda: mm.Un(X.astype(np.float32), Z, **E), lambda: mm.Un(X, Z.astype(np.int64), **G),
        lambda: mm.Un(X[:, ::2], Z[:, ::2], **E), lambda: mm.components(X.T, Z.T, **G),
        lambda: mm.Un(X.reshape(5, 2, 4), Z, **E), lambda: mm.UB(X, Z.reshape(3, 2, 4), 5, **G),
        lambda: mm.Un(x1[::2], x1, **E),
        # d: a mismatch, above 64, none
        lambda: mm.Un(X, x1, **E), lambda: mm.Un(wide, wide, **G), lambda: mm.UB(wide, wide, 3, **E),
        lambda: mm.Un(np.zeros((4, 0)), np.zeros((3, 0)), **E),
        # too few rows
        lambda: mm.Un(X[:1], Z, **E), lambda: mm.Un(X, Z[:1], **G), lambda: mm.components(X[:0], Z, **E),
        lambda: mm.UB(X, Z[:1], 4, **E), lambda: mm.UB_indices(X[:1], Z, [0], [0], [0], [1], **G),
        # the kernel and its sigma
        lambda: mm.Un(X, Z, kernel="laplace", sigma=1.0), lambda: mm.UB(X, Z, 3, kernel=None),
        lambda: mm.Un(X, Z), lambda: mm.Un(X, Z, kernel="gaussian"), lambda: mm.UB(X, Z, 3),
        lambda: mm.Un(X, Z, sigma=0.0), lambda: mm.Un(X, Z, sigma=-1.0),
        lambda: mm.components(X, Z, sigma=float("nan")), lambda: mm.UB(X, Z, 3, sigma=float("inf")),
        lambda: mm.Un(X, Z, sigma="wide"), lambda: mm.Un(X, Z, sigma=1e-200),
        lambda: mm.Un(X, Z, kernel="energy", sigma=1.0), lambda: mm.UB(X, Z, 3, kernel="energy", sigma=2),
        lambda: mm.UnN(X, Z, 2), lambda: mm.UnNB(X, Z, 2, 3, sigma=0.0),
        lambda: mm.UnNT(X, Z, 2, 2, kernel="energy", sigma=1.0), lambda: mm.UnNBT(X, Z, 2, 3, 2, kernel="x"),
        # index arrays of different shapes; i == j, k == l (also through a negative index)
        lambda: mm.UB_indices(X, Z, [0, 1], [1], [0, 0], [1, 1], **E),
        lambda: mm.UB_indices(X, Z, [0, 1], [1, 0], [0, 1], [1], **G),
        lambda: mm.UB_indices(X, Z, [0, 3], [1, 3], [0, 1], [1, 0], **E),
        lambda: mm.UB_indices(X, Z, [0, 3], [1, 2], [0, 1], [1, 1], **G),
        lambda: mm.UB_indices(X, Z, [0, -1], [1, 9], [0, 1], [1, 0], **E),
        lambda: mm.UB_indices(X, Z, [0], [1], [5], [-1], **E),
        # partitions out of scope
        lambda: mm.UnN(X, Z, 2, "SWOR", **E), lambda: mm.UnNB(X, Z, 2, 3, "prop-SWR", **G),
        lambda: mm.UnNT(X, Z, 2, 2, "SWR", **E), lambda: mm.UnNBT(X, Z, 2, 3, 2, "SWOR", **G),
        lambda: mm.UN(X, Z, 2, lambda x, z: 0.0, "SWOR"),
        # a block of fewer than 2 rows of X or of Z
        lambda: mm.UnN(X, Z, 6, **E), lambda: mm.UnN(X, Z, 4, **G), lambda: mm.UnNT(X, Z, 7, 2, **E),
        lambda: mm.UnNB(X, Z, 4, 3, **E), lambda: mm.UnNBT(X, Z, 7, 3, 2, **G),
        lambda: mm.UN(X, Z, 4, lambda x, z: 0.0),
        # UN shuffles in place: lists are refused
        lambda: mm.UN(X.tolist(), Z, 2, lambda x, z: 0.0), lambda: mm.UN(X, Z.tolist(), 2, lambda x, z: 0.0),
    ]
    for n, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert same_state(np.random.get_state(), state), n
    with pytest.raises(ValueError, match="prop-SWOR"):
        mm.UnN(X, Z, 2, "SWOR", **E)
    with pytest.raises(ValueError, match="needs sigma"):
        mm.Un(X, Z)
    with pytest.raises(ValueError, match="i != j and k != l"):
        mm.UB_indices(X, Z, [2], [2], [0], [1], **E)
    # rows out of range are NumPy's IndexError, as in the sibling modules
    for call in (lambda: mm.UB_indices(X, Z, [10], [0], [0], [1], **E),
                 lambda: mm.UB_indices(X, Z, [0], [-11], [0], [1], **E),
                 lambda: mm.UB_indices(X, Z, [0], [1], [6], [0], **G),
                 lambda: mm.UB_indices(X, Z, [0], [1], [0], [-7], **G),
                 lambda: mm.UB_indices(X, Z, [0.0], [1], [0], [1], **E)):
        with pytest.raises(IndexError):
            call()
    # nothing was shuffled and nothing was drawn on the way to those errors
    assert np.array_equal(X, X0) and np.array_equal(Z, Z0)
    assert same_state(np.random.get_state(), state)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.mmd as mm
    X, Z = data("gauss", 6, 4, 3, 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        mm.Un(X, Z, sigma=1.0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        mm.components(X, Z, kernel="energy")
    with pytest.raises(RuntimeError, match="no HIP device"):
        mm.UB_indices(X, Z, [0, 1], [2, 3], [0, 1], [1, 0], kernel="energy")


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")

    def sums(d=3, n_blocks=1, max_n=2, max_m=2, kern=L.TW_MMD_GAUSSIAN, c=-0.5, ptr=p, out=p):
        return lib.tw_mmd_sums(p, ptr, d, p, p, n_blocks, max_n, max_m, kern, c, p, out, None)

    def idx(d=3, n_shards=1, max_q=4, kern=L.TW_MMD_ENERGY, c=0.0, ptr=p):
        return lib.tw_mmd_idx32(p, p, d, p, p, p, ptr, p, n_shards, max_q, kern, c, p, p, None)

    for name, fn in ((b"tw_mmd_sums", sums), (b"tw_mmd_idx32", idx)):
        G = dict(kern=L.TW_MMD_GAUSSIAN)
        for call, word in ((lambda: fn(ptr=None), b"null pointer"),
                           (lambda: fn(d=0), b"outside [1, 64]"),
                           (lambda: fn(d=65), b"outside [1, 64]"),
                           (lambda: fn(kern=2), b"unknown kernel"),
                           (lambda: fn(kern=-1), b"unknown kernel"),
                           (lambda: fn(c=0.5, **G), b"Gaussian"),
                           (lambda: fn(c=nan, **G), b"Gaussian"),
                           (lambda: fn(c=-inf, **G), b"Gaussian"),
                           (lambda: fn(c=inf, **G), b"Gaussian")):
            assert call() == L.TW_ERR_ARG, (name, word)
            msg = lib.tw_last_error()
            assert word in msg and name in msg, msg
    for call in (lambda: sums(out=None), lambda: sums(n_blocks=-1), lambda: sums(max_n=-1),
                 lambda: sums(max_m=-2), lambda: idx(n_shards=-1), lambda: idx(max_q=-1)):
        assert call() == L.TW_ERR_ARG
        msg = lib.tw_last_error()
        assert b"negative size" in msg or b"null pointer" in msg, msg
    # nothing to do: no blocks, no shards (the energy kernel ignores c)
    assert sums(n_blocks=0) == L.TW_OK and idx(n_shards=0, c=nan) == L.TW_OK
    with pytest.raises(ValueError, match="unknown kernel"):
        L.call("tw_mmd_sums", p, p, 3, p, p, 1, 2, 2, 7, -0.5, p, p, None)
    P = lib.tw_mmd_tile()
    assert 64 <= P <= 4096 and P % 64 == 0
    small, big = lib.tw_mmd_work_bytes(1, 2, 2), lib.tw_mmd_work_bytes(64, 1562, 1562)
    assert 24 <= small <= big < 1 << 26 and lib.tw_mmd_work_bytes(-1, 1, 1) == 0
    assert lib.tw_mmd_work_bytes(1, -1, 1) == 0 and lib.tw_mmd_work_bytes(1, 1, -1) == 0
    assert big % 24 == 0  # three doubles per workgroup
    small, big = lib.tw_mmd_idx_work_bytes(1, 1), lib.tw_mmd_idx_work_bytes(64, 10 ** 6)
    assert 32 <= small <= big < 1 << 26 and lib.tw_mmd_idx_work_bytes(-1, 1) == 0
