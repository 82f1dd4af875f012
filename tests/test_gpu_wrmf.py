"""WRMF on the GPU (include/wrmf.h, wrmf.hip) against the reference's own results
(tests/golden/wrmf_cases.npz), rounding-error bounds and the numpy restatement (wrmf_numpy.py).

Reference parity is max|GPU - ref| / max|ref| <= 16 x the stored distance between the reference
(SuperLU) and the restatement (LAPACK Cholesky), floor 64 * 2^-53: the device is a third
backward-stable f64 algorithm on the same ill-conditioned systems, and every real defect (f32
anywhere, the wrong Gram matrix, a missing lambda, a dropped chunk) lands at least 1e6 times
further out.
"""
import numpy as np
import pytest

import wrmf_numpy as W
from test_wrmf_cpu import ALPHA, CASES, LAMBDA, SEED, conf_of

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
LD = np.longdouble


def rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def check_parity(m, X_ref, Y_ref, dist_X, dist_Y, label):
    X, Y = m.factors()
    for tag, got, ref, dist in (("X", X, X_ref, dist_X), ("Y", Y, Y_ref, dist_Y)):
        r, bound = rel(got, ref), max(16 * dist, 64 * EPS)
        print(f"{label} {tag}: gpu-ref {r:.3e}  stored {dist:.3e}  bound {bound:.3e}")
        assert r <= bound, (label, tag, r, bound)


# ---- 1. reference parity -----------------------------------------------------------------------
@pytest.mark.parametrize("heavy", [0, 16])
@pytest.mark.parametrize("name", list(CASES))
def test_fit_matches_the_reference(rl, name, heavy):
    c = CASES[name]
    m = rl.WRMF(c["csr"], lambda_val=LAMBDA, alpha=ALPHA, iterations=c["epochs"], factor_num=c["d"],
                seed=SEED, heavy_nnz=heavy)
    m.fit()
    st = m.last_stats
    assert st["solves"] == c["epochs"] * (c["U"] + c["I"])
    assert (st["heavy_rows"] > 0) == (heavy == 16)  # row 7 has every other item: >= 24 entries
    check_parity(m, c["X"], c["Y"], c["dist_X"], c["dist_Y"], f"{name} heavy_nnz={heavy}")
    X, Y = m.factors()
    assert not X[3].any() and not np.signbit(X[3]).any()  # empty rows: exactly +0.0
    assert not Y[5].any() and not np.signbit(Y[5]).any()
    m.close()


# ---- 2. Gram -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 20, 128])
@pytest.mark.parametrize("n", [1, 47, 5000])
def test_gram_within_the_dot_product_bound(rl, n, d):
    g = np.random.default_rng(100 * n + d)
    T = g.standard_normal((n, d)) * np.exp(g.standard_normal((n, 1)))
    empty = (np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), (n, 3))
    m = rl.WRMF(empty, factor_num=d)
    m.set_factors(T, np.zeros((3, d)))
    G1, G2 = m.gram(0), m.gram(0)
    assert np.array_equal(G1, G2)
    assert np.array_equal(G1, G1.T)
    TL = T.astype(LD)
    # the scale |T|^T |T| in f64 (its own relative error, ~1e-12, is nothing against the bound)
    exact, scale = TL.T @ TL, np.abs(T).T @ np.abs(T)
    ratio = float((np.abs(G1.astype(LD) - exact) / ((n + 2) * EPS * scale)).max())
    print(f"gram n={n} d={d}: max |dG| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert np.array_equal(m.gram(1), np.zeros((d, d)))
    m.close()


# ---- 3. half-sweep backward error --------------------------------------------------------------
SWEEP_U, SWEEP_I = 3000, 2000


def zipf_lognormal_csr(seed):
    """Zipf item popularity (the hottest item has a few thousand users), lognormal user activity."""
    g = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, SWEEP_I + 1)
    p /= p.sum()
    deg = np.clip(np.rint(np.exp(g.normal(3.0, 1.0, SWEEP_U))), 0, 600).astype(np.int64)
    deg[5] = 0
    indptr, cols, vals = np.zeros(SWEEP_U + 1, np.int64), [], []
    for u in range(SWEEP_U):
        it = np.unique(g.choice(SWEEP_I, size=deg[u], p=p)) if deg[u] else np.zeros(0, np.int64)
        cols.append(it)
        vals.append(g.integers(1, 6, len(it)))
        indptr[u + 1] = indptr[u] + len(it)
    return (indptr, np.concatenate(cols).astype(np.int32),
            ALPHA * np.concatenate(vals).astype(np.float64), (SWEEP_U, SWEEP_I))


def residual_ratios(conf, T_in, G, lam, sols, b_terms=False):
    """Per row and per solution in `sols`: |A x - b|_inf / (gamma (|A|_inf |x|_inf + |b|_inf)),
    gamma = (d (3 d + 1) + nnz + 2) 2^-53.  A x is applied in long double from the inputs and the
    device's own G as G x + Tn^T (c o (Tn x)) + lam x; |A|_inf comes from the f64 matrix (relative
    error ~1e-13, nothing against the bound's headroom).  b_terms: |b|_inf is replaced by
    max_j sum_n |(c_n + 1) t_nj|, the quantity the accumulation error of b is actually relative to
    (|b^ - b| <= nnz 2^-53 sum_n |(c_n + 1) t_n|); the two agree unless b's terms cancel."""
    indptr, indices, data, (n, _) = conf
    d = T_in.shape[1]
    GL, TL = G.astype(LD), T_in.astype(LD)
    out = np.zeros((len(sols), n))
    for r in range(n):
        sl = slice(indptr[r], indptr[r + 1])
        nnz = sl.stop - sl.start
        if nnz == 0:
            for s, x in enumerate(sols):
                out[s, r] = 0.0 if not x[r].any() else np.inf
            continue
        Tn, c = TL[indices[sl]], data[sl].astype(LD)
        b = ((c + 1)[:, None] * Tn).sum(0)
        bnorm = np.abs((c + 1)[:, None] * Tn).sum(0).max() if b_terms else np.abs(b).max()
        A64 = G + (T_in[indices[sl]] * data[sl][:, None]).T @ T_in[indices[sl]] + lam * np.eye(d)
        normA = np.abs(A64).sum(1).max()
        gamma = (d * (3 * d + 1) + nnz + 2) * EPS
        for s, x in enumerate(sols):
            xl = x[r].astype(LD)
            res = GL @ xl + Tn.T @ (c * (Tn @ xl)) + LD(lam) * xl - b
            out[s, r] = float(np.abs(res).max() / (gamma * (normA * np.abs(xl).max() + bnorm)))
    return out


@pytest.fixture(scope="module", params=[20, 64])
def sweeps(rl, request):
    """Both half-sweeps at the default heavy_nnz and at 64, and every row's residual ratio."""
    d = request.param
    conf = zipf_lognormal_csr(7)
    conf_t = W.transpose_csr(conf)
    hottest = int(np.diff(conf_t[0]).max())
    assert 1000 < hottest <= SWEEP_U
    g = np.random.default_rng(d)
    X0, Y0 = g.standard_normal((SWEEP_U, d)), g.standard_normal((SWEEP_I, d))
    got = {}
    for heavy in (0, 64):
        m = rl.WRMF((conf[0], conf[1], conf[2] / ALPHA, conf[3]), lambda_val=LAMBDA, alpha=ALPHA,
                    factor_num=d, heavy_nnz=heavy)
        m.set_factors(X0, Y0)
        Gy = m.gram(1)
        st0 = m.sweep(0)
        X1, _ = m.factors()
        Gx = m.gram(0)
        st1 = m.sweep(1)
        _, Y1 = m.factors()
        got[heavy] = dict(Gy=Gy, Gx=Gx, X1=X1, Y1=Y1, st=(st0, st1))
        m.close()
    assert np.array_equal(got[0]["Gy"], got[64]["Gy"])
    ru = residual_ratios(conf, Y0, got[0]["Gy"], LAMBDA, [got[0]["X1"], got[64]["X1"]])
    ri = [residual_ratios(conf_t, got[h]["X1"], got[h]["Gx"], LAMBDA, [got[h]["Y1"]])[0] for h in (0, 64)]
    return dict(d=d, got=got, ratios={0: (ru[0], ri[0]), 64: (ru[1], ri[1])},
                nnz=(np.diff(conf[0]), np.diff(conf_t[0])))


@pytest.mark.parametrize("heavy", [0, 64])
def test_half_sweep_backward_error_of_every_row(sweeps, heavy):
    ru, ri = sweeps["ratios"][heavy]
    st0, st1 = sweeps["got"][heavy]["st"]
    print(f"d={sweeps['d']} heavy_nnz={heavy}: max residual / bound users {ru.max():.4f} "
          f"items {ri.max():.4f}; heavy rows {st0['heavy_rows']} + {st1['heavy_rows']}")
    nu, ni = sweeps["nnz"]
    assert st0["solves"] == SWEEP_U and st1["solves"] == SWEEP_I
    if heavy:
        assert st0["heavy_rows"] == int((nu > heavy).sum()) > 0
        assert st1["heavy_rows"] == int((ni > heavy).sum()) > 0
    else:
        assert st0["heavy_rows"] == st1["heavy_rows"] == 0
    assert ru.shape == (SWEEP_U,) and ri.shape == (SWEEP_I,)
    assert (ru <= 1.0).all(), (int(np.argmax(ru)), float(ru.max()))
    assert (ri <= 1.0).all(), (int(np.argmax(ri)), float(ri.max()))


# ---- 4. fresh mode -----------------------------------------------------------------------------
def test_fresh_mode_objective_never_increases(rl):
    c = CASES["c20"]
    conf = conf_of(c)
    m = rl.WRMF(c["csr"], lambda_val=LAMBDA, alpha=ALPHA, factor_num=c["d"], seed=SEED, gram="fresh")
    obj = [W.objective(conf, *m.factors(), LAMBDA)]
    for half in range(8):
        side = half % 2
        m.gram(1 - side)
        m.sweep(side)
        obj.append(W.objective(conf, *m.factors(), LAMBDA))
    print("objective:", " ".join(f"{o:.6e}" for o in obj))
    for a, b in zip(obj, obj[1:]):
        assert b <= a * (1 + 1e-12), obj
    m.close()


def test_fresh_mode_fit_matches_the_fresh_restatement(rl):
    c = CASES["c20"]
    Xn, Yn = W.fit(conf_of(c), c["X0"], c["Y0"], LAMBDA, c["epochs"], gram="fresh")
    m = rl.WRMF(c["csr"], lambda_val=LAMBDA, alpha=ALPHA, iterations=c["epochs"], factor_num=c["d"],
                seed=SEED, gram="fresh").fit()
    check_parity(m, Xn, Yn, c["dist_X"], c["dist_Y"], "c20 fresh")
    assert np.abs(m.factors()[0] - c["X"]).max() > 1.0  # and far from the reference mode's result
    m.close()


# ---- 5. determinism and surface ----------------------------------------------------------------
@pytest.mark.parametrize("heavy", [0, 16])
def test_two_fits_give_identical_bits(rl, heavy):
    c = CASES["c32"]
    res = []
    for _ in range(2):
        m = rl.WRMF(c["csr"], lambda_val=LAMBDA, alpha=ALPHA, iterations=c["epochs"],
                    factor_num=c["d"], seed=SEED, heavy_nnz=heavy).fit()
        res.append(m.factors())
        m.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_predict_and_the_reference_drivers_product(rl):
    c = CASES["c20"]
    m = rl.WRMF(c["csr"], lambda_val=LAMBDA, alpha=ALPHA, iterations=1, factor_num=c["d"], seed=SEED).fit()
    X, Y = m.factors()
    g = np.random.default_rng(0)
    us, it = g.integers(0, c["U"], 200), g.integers(0, c["I"], 200)
    want = np.einsum("nd,nd->n", X[us], Y[it])
    np.testing.assert_allclose(m.predict_batch(us, it), want, rtol=1e-12, atol=0)
    p = m.predict(int(us[0]), int(it[0]))
    assert isinstance(p, float)
    np.testing.assert_allclose(p, want[0], rtol=1e-12, atol=0)
    assert m.predict(3, 0) == 0.0  # the empty user
    for u, i in ((-1, 0), (c["U"], 0), (0, -1), (0, c["I"])):
        with pytest.raises(IndexError):
            m.predict(u, i)
        with pytest.raises(IndexError):
            m.predict_batch([0, u], [0, i])
    rates = m.user_vec[7, :].dot(m.item_vec).toarray()  # WRMFRecommender.py:147, :179
    assert rates.shape == (1, c["I"])
    np.testing.assert_allclose(rates[0], X[7] @ Y.T, rtol=1e-12, atol=1e-300)
    assert m.user_vec.shape == (c["U"], c["d"]) and m.item_vec.shape == (c["d"], c["I"])
    m.close()


def test_documented_failures(rl):
    c = CASES["c8"]
    with pytest.raises(rl.BprmfError, match="error -6"):  # BPRMF_E_UNSUPPORTED
        rl.WRMF(c["csr"], factor_num=129)
    with pytest.raises(rl.BprmfError, match="error -6"):
        rl.WRMF(c["csr"], factor_num=0)
    indptr, indices, data, shape = c["csr"]
    bad = indices.copy()
    b, e = indptr[7], indptr[8]
    bad[b], bad[b + 1] = indices[b + 1], indices[b]
    with pytest.raises(ValueError, match="strictly increasing"):  # BPRMF_E_RANGE
        rl.WRMF((indptr, bad, data, shape), factor_num=8)
    dup = indices.copy()
    dup[b + 1] = dup[b]
    with pytest.raises(ValueError, match="strictly increasing"):
        rl.WRMF((indptr, dup, data, shape), factor_num=8)
    far = indices.copy()
    far[e - 1] = shape[1]
    with pytest.raises(ValueError, match="out of range"):
        rl.WRMF((indptr, far, data, shape), factor_num=8)


@pytest.mark.parametrize("d", [1, 16, 17, 100])
def test_any_factor_count_solves_within_the_backward_error_bound(rl, d):
    """d below, at and just past the 16-wide tile and at an odd tile count, on the c8 ratings with
    unit-scale factors: both half-sweeps under the bound of the half-sweep test, every row.

    The right-hand side enters the bound by its terms (residual_ratios b_terms): at d = 1 a row's
    b = sum (c + 1) y can cancel (row 6 here: b = 0.75 from terms of 297 in all), |A| |x| is then
    no larger than |b|, and the rounding of the sum alone exceeds gamma |b|.  The numpy
    restatement sits at 7.3 x the |b|-based bound on that row, so that form cannot hold for any
    f64 code; with d >= 16 the |A| |x| term covers it and both forms pass."""
    c = CASES["c8"]
    conf = conf_of(c)
    conf_t = W.transpose_csr(conf)
    g = np.random.default_rng(d)
    X0, Y0 = g.standard_normal((c["U"], d)), g.standard_normal((c["I"], d))
    for heavy in (0, 16):
        m = rl.WRMF(c["csr"], lambda_val=LAMBDA, alpha=ALPHA, factor_num=d, heavy_nnz=heavy)
        m.set_factors(X0, Y0)
        Gy = m.gram(1)
        m.sweep(0)
        X1, _ = m.factors()
        Gx = m.gram(0)
        m.sweep(1)
        _, Y1 = m.factors()
        m.close()
        ru = residual_ratios(conf, Y0, Gy, LAMBDA, [X1], b_terms=True)[0]
        ri = residual_ratios(conf_t, X1, Gx, LAMBDA, [Y1], b_terms=True)[0]
        print(f"d={d} heavy_nnz={heavy}: max residual / bound users {ru.max():.4f} items {ri.max():.4f}")
        assert (ru <= 1.0).all() and (ri <= 1.0).all()


def test_predict_staging_regrows_and_a_failed_set_train_keeps_the_train_set(rl):
    """predict_batch with 1, 300 and 2 pairs on one handle (the staging grows once and is then
    reused); a refused wrmf_set_train on that handle leaves the previous train set whole."""
    g = np.random.default_rng(3)
    U, I, d = 6, 5, 4
    dense = g.integers(1, 6, (U, I)) * (g.random((U, I)) < 0.6)
    dense[2] = 0  # an empty user
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(1))]).astype(np.int64)
    indices = np.nonzero(dense)[1].astype(np.int32)
    csr = (indptr, indices, dense[dense != 0].astype(np.float64), (U, I))
    make = lambda: rl.WRMF(csr, lambda_val=LAMBDA, alpha=ALPHA, iterations=2, factor_num=d, seed=SEED)  # noqa: E731
    m = make().fit()
    X, Y = m.factors()
    for n in (1, 300, 2):
        us, it = g.integers(0, U, n), g.integers(0, I, n)
        np.testing.assert_allclose(m.predict_batch(us, it), np.einsum("nd,nd->n", X[us], Y[it]),
                                   rtol=1e-12, atol=0)
    b = int(np.argmax(np.diff(indptr) >= 2))  # a row with two entries: swap them
    bad = indices.copy()
    bad[indptr[b]], bad[indptr[b] + 1] = indices[indptr[b] + 1], indices[indptr[b]]
    conf = np.ascontiguousarray(ALPHA * csr[2])
    with pytest.raises(ValueError, match="strictly increasing"):
        rl._lib.check(m._L.wrmf_set_train(m._h, rl._lib.ptr(indptr), rl._lib.ptr(bad),
                                          rl._lib.ptr(conf), len(bad)))
    m.fit()
    fresh = make().fit().fit()
    for got, want in zip(m.factors(), fresh.factors()):
        assert np.array_equal(got, want)
    m.close()
    fresh.close()
