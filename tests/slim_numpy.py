"""NumPy restatement of the reference's SLIM (util/slim.pyx:43-126, SLiMRecommender.py:42-46, :123):
both coordinate-descent variants with the reference's operation order, and the scores A.W summed
in ascending item order.  Everything is IEEE double with separate multiplies and adds, which is
what the compiled reference executes, so `fit` gives the reference's W bit for bit
(tests/golden/make_golden_slim.py asserts it when it writes the fixtures).

The scan over j evaluates a block of candidates against the current gradient components and
applies the first one that moves; the candidates before it did not move under the values they
saw and the ones after it are evaluated again, so every g[k] and w[j] sees the reference's
operations in the reference's order.  The update over k is `g += G[:, j] * delta`: NumPy
multiplies, then adds.

Besides W, `fit` returns what the reference does not expose, per column: the sweeps it ran (of
both modes), its moves, and whether it ran max_iter sweeps (never with max_iter = 0, when no sweep runs).
"""
import numpy as np

BLOCK = 128


def dense(pairs, U, p):
    """A [U, p] of 0/1 (SLiMRecommender.py:42-46): duplicate pairs collapse."""
    A = np.zeros((U, p))
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    A[pairs[:, 0], pairs[:, 1]] = 1.0
    return A


def csr(pairs, U, p):
    """(indptr int64 [U + 1], indices int32) of A: items ascending within a user, no duplicates."""
    A = dense(pairs, U, p)
    u, i = np.nonzero(A)
    return np.concatenate([[0], np.cumsum(np.bincount(u, minlength=U))]).astype(np.int64), i.astype(np.int32)


def gram(pairs, U, p):
    """G = A^T A as the exact integer counts, in f64."""
    A = dense(pairs, U, p).astype(np.int64)
    return (A.T @ A).astype(np.float64)


def penalties(Gc, col, alpha, lam, ratio, N):
    """(b, c) of one column, or None where the ratio variant leaves the column zero (:90-98)."""
    if not ratio:
        return lam * alpha * N, lam * (1 - alpha) * N  # :45-46
    m = Gc.copy()
    m[col] = 0.0
    max_cov = max(0.0, float(m.max()))
    if max_cov == 0:
        return None
    return max_cov * lam, max_cov * (1 - alpha) / alpha * lam


def fit_column(G, diag, col, alpha, lam, ratio, max_iter, tol, N):
    """One column of W: (w [p], sweeps, moves, capped)."""
    p = G.shape[0]
    w, g = np.zeros(p), np.zeros(p)
    Gc = G[col]  # = G[:, col]: G is symmetric
    bc = penalties(Gc, col, float(alpha), float(lam), ratio, float(N))
    if bc is None:
        return w, 0, 0, 0
    b, c = bc
    den = c + diag
    mode = sweeps = moves = 0
    for _ in range(max_iter):
        sweeps += 1
        move, j0 = False, 0
        while j0 < p:
            j1 = min(p, j0 + BLOCK)
            wj = w[j0:j1]
            a = (Gc[j0:j1] + diag[j0:j1] * wj) - g[j0:j1]
            s = np.where((b >= np.abs(a)) | (a <= 0), 0.0, a - b)
            new = s / den[j0:j1]  # 0/0 = NaN where nobody rated j and c == 0: no move
            delta = new - wj
            mv = np.abs(delta) > tol
            if j0 <= col < j1:
                mv[col - j0] = False
            if mode == 1:
                mv &= wj != 0
            if not mv.any():
                j0 = j1
                continue
            r = int(mv.argmax())
            j = j0 + r
            w[j] = new[r]
            g += G[j] * delta[r]
            moves += 1
            move = True
            j0 = j + 1
        if not move:
            if mode == 0:
                break
            mode = 0
        elif mode == 0:
            mode = 1
    return w, sweeps, moves, int(max_iter > 0 and sweeps == max_iter)


def fit(G, alpha, lam, ratio, max_iter, tol, N, columns=None):
    """(W [p, end - begin], counters [end - begin, 3] = sweeps, moves, capped per column)."""
    p = G.shape[0]
    begin, end = (0, p) if columns is None else columns
    G = np.ascontiguousarray(G, np.float64)
    diag = np.ascontiguousarray(np.diag(G))
    W = np.zeros((p, end - begin))
    counters = np.zeros((end - begin, 3), np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for col in range(begin, end):
            w, sweeps, moves, capped = fit_column(G, diag, col, alpha, lam, ratio, max_iter, tol, N)
            W[:, col - begin] = w
            counters[col - begin] = sweeps, moves, capped
    return W, counters


def score_rows(indptr, indices, W, users):
    """Rows of A.W: the user's W[j, :] rows added one by one in ascending j, from +0.0."""
    out = np.zeros((len(users), W.shape[1]))
    for n, u in enumerate(users):
        for j in indices[indptr[u]:indptr[u + 1]]:
            out[n] += W[j]
    return out


def scores(indptr, indices, W, users, items):
    out = np.zeros(len(users))
    for n, (u, i) in enumerate(zip(users, items)):
        acc = 0.0
        for j in indices[indptr[u]:indptr[u + 1]]:
            acc += W[j, i]
        out[n] = acc
    return out


def rank(score, k):
    """Positions of the k best of one list: score descending, ties by the earlier position."""
    return np.argsort(-np.asarray(score, np.float64), kind="stable")[:k]
