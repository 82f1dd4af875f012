"""Dense numpy restatement of the reference's WRMF epoch (WRMFRecommender.py:37-58); a test
helper, not a test.  Every row is one d x d symmetric positive-definite system

    (G + sum_n c_n t_n t_n^T + lam I) x = sum_n (c_n + 1) t_n

over the row's non-zero entries n (c = alpha * rating, t_n the neighbour's factor row, G the Gram
matrix of the whole neighbour table), solved with np.linalg.cholesky.  gram="reference" takes
both Gram matrices before the user sweep, as the reference does (the item sweep then sees the
XtX of the old X); gram="fresh" recomputes XtX after the user sweep (textbook ALS).
"""
import numpy as np


def as_csr(m):
    """(indptr int64, indices int32, data float64, shape) of a SciPy matrix or such a tuple, column
    indices sorted within each row."""
    if isinstance(m, tuple):
        indptr, indices, data, shape = m
    else:
        m = m.tocsr().copy()
        m.sum_duplicates()
        m.sort_indices()
        indptr, indices, data, shape = m.indptr, m.indices, m.data, m.shape
    return (np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32),
            np.ascontiguousarray(data, np.float64), (int(shape[0]), int(shape[1])))


def transpose_csr(csr):
    """The by-column structure of a CSR tuple, rows of the result sorted by original row."""
    indptr, indices, data, (U, I) = csr
    rows = np.repeat(np.arange(U, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    tptr = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(indices, minlength=I), out=tptr[1:])
    return tptr, rows[order].astype(np.int32), data[order], (I, U)


def row_system(conf_csr, T_in, G, lam, r, dtype=np.float64):
    """(A, b) of row r; entries with a zero confidence do not count (the reference's Pu != 0)."""
    indptr, indices, data, _ = conf_csr
    d = T_in.shape[1]
    sl = slice(indptr[r], indptr[r + 1])
    c = np.asarray(data[sl], dtype)
    Tn = np.asarray(T_in[indices[sl]], dtype)[c != 0]
    c = c[c != 0]
    A = np.asarray(G, dtype) + (Tn * c[:, None]).T @ Tn + np.asarray(lam, dtype) * np.eye(d, dtype=dtype)
    b = ((c + 1)[:, None] * Tn).sum(0)
    return A, b, len(c)


def half_sweep(conf_csr, T_in, G, lam):
    """Solve every row of conf_csr against the neighbour table T_in and its Gram matrix G."""
    n, d = conf_csr[3][0], T_in.shape[1]
    out = np.zeros((n, d))
    for r in range(n):
        A, b, nnz = row_system(conf_csr, T_in, G, lam, r)
        if nnz == 0:
            continue
        L = np.linalg.cholesky(A)
        out[r] = np.linalg.solve(L.T, np.linalg.solve(L, b))
    return out


def fit(conf_csr, X, Y, lam, epochs, gram="reference"):
    """`epochs` epochs from (X, Y); returns the new (X, Y)."""
    assert gram in ("reference", "fresh")
    conf_t = transpose_csr(conf_csr)
    X, Y = X.copy(), Y.copy()
    for _ in range(epochs):
        yTy = Y.T @ Y
        xTx = X.T @ X
        X = half_sweep(conf_csr, Y, yTy, lam)
        if gram == "fresh":
            xTx = X.T @ X
        Y = half_sweep(conf_t, X, xTx, lam)
    return X, Y


def objective(conf_csr, X, Y, lam):
    """sum_{u,i} (1 + C_ui)(p_ui - x_u.y_i)^2 + lam (|X|^2 + |Y|^2), dense."""
    indptr, indices, data, (U, I) = conf_csr
    C = np.zeros((U, I))
    rows = np.repeat(np.arange(U), np.diff(indptr))
    C[rows, indices] = data
    P = (C != 0).astype(np.float64)
    R = P - X @ Y.T
    return float(((1.0 + C) * R * R).sum() + lam * ((X * X).sum() + (Y * Y).sum()))
