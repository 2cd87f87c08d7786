"""Plain reference of the KKT linear algebra: a right-looking L D L' without pivoting and the
unit-lower substitutions, generic in the number format (float64 and the 80-bit
``numpy.longdouble``), and the 80-bit evaluation of ``L D L'``, ``|L||D||L'|`` and residuals
that the backward-error bounds of tests/test_gpu_linalg.py are checked with.  Written from
the textbook algorithm (Golub & Van Loan 4.1.2; Higham, Accuracy and Stability, ch. 10), not
from the device code."""
import numpy as np

F64 = np.float64
F80 = np.longdouble
U = 2.0 ** -53      # unit roundoff of binary64


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


def ldl(K, dtype=F64):
    """(L, D, fail): K = L diag(D) L' with L unit lower, by the right-looking elimination on
    the lower triangle, in ``dtype``.  fail is the index of the first pivot that is not
    positive and finite (the factorisation stops there), else None."""
    A = np.array(K, dtype=dtype)
    n = A.shape[0]
    L = np.eye(n, dtype=dtype)
    D = np.zeros(n, dtype=dtype)
    for j in range(n):
        d = A[j, j]
        if not (np.isfinite(d) and d > 0):
            return L, D, j
        D[j] = d
        if j + 1 < n:
            c = A[j + 1:, j].copy()
            l = c / d
            L[j + 1:, j] = l
            A[j + 1:, j + 1:] -= np.tril(np.outer(l, c))
    return L, D, None


def solve(L, D, b, dtype=F64):
    """x of L diag(D) L' x = b by forward substitution, scaling and backward substitution."""
    n = L.shape[0]
    L = L.astype(dtype)
    y = np.array(b, dtype=dtype)
    for j in range(n):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    y = y / D.astype(dtype)
    for j in range(n - 1, -1, -1):
        y[:j] -= L[j, :j] * y[j]
    return y


def products(L, D):
    """(L D L', |L||D||L'|) evaluated in 80-bit."""
    L = L.astype(F80)
    D = np.asarray(D, dtype=F80)
    aL = np.abs(L)
    return (L * D) @ L.T, (aL * np.abs(D)) @ aL.T


def _ratio(res, bound):
    """res / bound entrywise; where the bound is zero (a structural zero of K with no
    products under it) a zero residual counts 0 and any other infinity."""
    out = np.where(res == 0, F80(0), F80(np.inf))
    np.divide(res, bound, out=out, where=bound > 0)
    return out


def factor_ratio(K, L, dinv, prods=None):
    """max over the lower triangle of |K - L D L'| / (gamma(n + 1) |L||D||L'|) with D = 1 / dinv
    formed in 80-bit: the componentwise backward error of a factorisation in units of
    Higham's bound (Theorem 10.3's proof holds for any order of the sums)."""
    n = K.shape[0]
    P, Pa = prods if prods is not None else products(L, F80(1) / np.asarray(dinv, dtype=F80))
    return float(np.max(np.tril(_ratio(np.abs(np.asarray(K, dtype=F80) - P), F80(gamma(n + 1)) * Pa))))


def solve_ratio(L, dinv, b, x, prods=None):
    """max_i |b - L D L' x|_i / (gamma(3 n + 1) (|L||D||L'||x|)_i) in 80-bit: the solve's
    backward error with the given factor, in units of the bound for the two substitutions and
    the scaling (Higham Theorem 8.5 applied to L, D and L')."""
    n = L.shape[0]
    if prods is None:
        prods = products(L, F80(1) / np.asarray(dinv, dtype=F80))
    P, Pa = prods
    x = np.asarray(x, dtype=F80)
    return float(np.max(_ratio(np.abs(np.asarray(b, dtype=F80) - P @ x),
                               F80(gamma(3 * n + 1)) * (Pa @ np.abs(x)))))


def full_lower(K):
    """The symmetric matrix whose lower triangle is K's."""
    T = np.tril(K)
    return T + np.tril(K, -1).T
