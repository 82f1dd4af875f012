"""SLIM on the GPU (include/slim.h, slim.hip) against the compiled reference's own results
(tests/golden/slim_cases.npz) and the numpy restatement (slim_numpy.py).

Nothing here has a tolerance of its own: the Gram matrix is integer counts and must be exact, W
must equal the reference bit for bit on the LDS path, the workspace path and as two column
ranges, the scores must equal the restatement's sequential sums exactly and the fixture's
A.dot(W) within the summation bound of test_slim_cpu.py.
"""
import numpy as np
import pytest

import slim_numpy as S
from test_slim_cpu import CASES, SETTINGS, score_bound

pytestmark = pytest.mark.gpu
TOTALS = ("sweeps", "moves", "capped")


def model(rl, c, **kw):
    return rl.SLIM(c["pairs"], num_user=c["U"], num_item=c["p"], **kw)


def fit(m, s, columns=None):
    m.fit(alpha=s["alpha"], lam_bda=s["lam"], max_iter=s["max_iter"], tol=s["tol"],
          lambda_is_ratio=s["ratio"], columns=columns)
    return m.last_stats


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def check_fit(st, W, s, begin, end, label):
    want = s["counters"][begin:end].sum(0)
    got = [st[k] for k in TOTALS]
    diff = int((W.view(np.int64) != s["W"].view(np.int64))[:, begin:end].sum())
    print(f"{label}: columns {begin}:{end}  differing entries {diff}  sweeps/moves/capped {got} want {want.tolist()}")
    assert diff == 0, label
    assert got == want.tolist(), label
    assert st["columns"] == end - begin


@pytest.fixture(scope="module")
def fitted(rl):
    """One fitted model per fixture and setting (the LDS path), shared by the read-only tests."""
    made = {}

    def get(name, tag):
        if (name, tag) not in made:
            m = model(rl, CASES[name])
            fit(m, CASES[name]["settings"][tag])
            made[name, tag] = m
        return made[name, tag]
    yield get
    for m in made.values():
        m.close()


# ---- 1. Gram -----------------------------------------------------------------------------------
@pytest.mark.parametrize("U,p", [(1, 1), (63, 31), (65, 33), (130, 257), (1000, 96)])
def test_gram_is_exact(rl, U, p):
    g = np.random.default_rng(1000 * U + p)
    A = g.random((U, p)) < 0.2
    A[U // 2, :] = True  # a user with every item
    u, i = np.nonzero(A)
    pairs = np.stack([u, i], axis=1)
    pairs = np.concatenate([pairs, pairs[::3]])[g.permutation(len(pairs) + len(pairs[::3]))]  # duplicates
    m = rl.SLIM(pairs, num_user=U, num_item=p)
    G = m.gram()
    A64 = A.astype(np.int64)
    want = A64.T @ A64
    assert G.dtype == np.float64 and G.shape == (p, p)
    assert np.array_equal(G, want.astype(np.float64))
    assert np.array_equal(G, G.T)
    assert np.array_equal(G, S.gram(pairs, U, p))
    assert np.array_equal(m.gram(), G)
    assert not m.W.any()  # gram() leaves W zero
    m.close()


def test_gram_of_the_fixtures(rl):
    for c in CASES.values():
        m = model(rl, c)
        assert np.array_equal(m.gram(), S.gram(c["pairs"], c["U"], c["p"]))
        m.close()


# ---- 2. fit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", SETTINGS)
def test_fit_equals_the_reference_bit_for_bit(fitted, name, tag):
    c, s = CASES[name], CASES[name]["settings"][tag]
    m = fitted(name, tag)
    check_fit(m.last_stats, m.W, s, 0, c["p"], f"{name} {tag} lds")
    assert not m.W[:, 5].any() and not m.W[5].any()  # the item nobody rated
    if s["ratio"]:
        assert not m.W[:, 11].any()  # max_cov == 0


@pytest.mark.parametrize("name,tag", SETTINGS)
def test_workspace_path_gives_the_same_bits(rl, name, tag):
    c, s = CASES[name], CASES[name]["settings"][tag]
    m = model(rl, c, chip_max_p=c["p"] - 1)
    st = fit(m, s)
    check_fit(st, m.W, s, 0, c["p"], f"{name} {tag} workspace")
    m.close()


@pytest.mark.parametrize("chip_max_p", [0, 16])
@pytest.mark.parametrize("name,tag", SETTINGS)
def test_two_column_ranges_and_a_second_fit(rl, name, tag, chip_max_p):
    c, s = CASES[name], CASES[name]["settings"][tag]
    p = c["p"]
    cut = (p // 2) | 1  # an odd column
    m = model(rl, c, chip_max_p=chip_max_p)
    st = fit(m, s, columns=(cut, p))
    W = m.W
    check_fit(st, W, s, cut, p, f"{name} {tag} upper range")
    assert not W[:, :cut].any()  # the other columns are untouched
    st = fit(m, s, columns=(0, cut))
    check_fit(st, m.W, s, 0, cut, f"{name} {tag} lower range")
    assert same_bits(m.W, s["W"])
    assert same_bits(m.weights((cut - 1, cut + 2)), s["W"][:, cut - 1:cut + 2])
    st = fit(m, s)  # a second fit of the same handle
    check_fit(st, m.W, s, 0, p, f"{name} {tag} second fit")
    m.close()


def test_max_iter_zero_and_one(rl):
    c = CASES["s60"]
    G = S.gram(c["pairs"], c["U"], c["p"])
    m = model(rl, c)
    for max_iter in (0, 1):
        m.fit(max_iter=max_iter)
        W, counters = S.fit(G, 0.5, 0.02, True, max_iter, 1e-4, c["U"])
        assert same_bits(m.W, W)
        assert [m.last_stats[k] for k in TOTALS] == counters.sum(0).tolist()
    m.fit(max_iter=0)
    assert m.last_stats["capped"] == 0 and not m.W.any()  # no sweep: nothing capped
    m.close()


# ---- 3. scores ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", SETTINGS)
def test_scores(fitted, name, tag):
    c, s = CASES[name], CASES[name]["settings"][tag]
    m = fitted(name, tag)
    users = c["aw_users"]
    rows = m.score_rows(users)
    want = S.score_rows(*c["csr"], s["W"], users)
    assert same_bits(rows, want)
    ref = s["aw"]
    excess = np.abs(rows - ref) - score_bound(c, users, ref)
    print(f"{name} {tag}: max |rows - A.dot(W)| = {np.abs(rows - ref).max():.3e}, worst excess over the bound {excess.max():.3e}")
    assert (excess <= 0).all()
    assert not rows[users == 3].any() and not np.signbit(rows[users == 3]).any()  # the empty user
    g = np.random.default_rng(5)
    sel = g.integers(0, len(users), 300)
    it = g.integers(0, c["p"], 300)
    got = m.predict_batch(users[sel], it)
    assert same_bits(got, want[sel, it])
    assert m.predict(int(users[sel[0]]), int(it[0])) == want[sel[0], it[0]]
    assert len(m.predict_batch([], [])) == 0 and m.score_rows([]).shape == (0, c["p"])


# ---- 4. ranking --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 32])
def test_recommend_is_a_stable_descending_ranking_of_the_device_scores(fitted, k):
    c = CASES["s700"]
    m = fitted("s700", "ratio")
    g = np.random.default_rng(k)
    users = np.array([7, 3, 9, 0, 1, 2, 50, 699, 7], np.int32)
    lens = [530, 400, 5, 0, 1, k - 1, 300, 1000, 33]  # unequal, empty, shorter than k, with repeats
    lists = [g.integers(0, c["p"], n).astype(np.int32) for n in lens]
    lists[0] = np.arange(c["p"], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = np.concatenate(lists)
    pos, score = m.recommend(users, offsets, items, k)
    zeros = 0
    for r, (u, lst) in enumerate(zip(users, lists)):
        sc = m.predict_batch(np.full(len(lst), u), lst)
        zeros += int((sc == 0).sum())
        want = S.rank(sc, k)
        n = len(want)
        assert pos[r, :n].tolist() == want.tolist(), r
        assert same_bits(score[r, :n], sc[want]), r
        assert (pos[r, n:] == -1).all() and np.isneginf(score[r, n:]).all(), r
    assert zeros >= 405  # many exact ties at 0: the whole lists of the empty and the isolated user


def test_ground_truth_gets_no_preference_among_tied_scores(rl):
    """Users whose every candidate scores exactly 0 (the empty user 3 and user 9, whose only item
    is isolated): the recommendation is the N smallest candidate ids, wherever the truth sits."""
    c, s = CASES["s60"], CASES["s60"]["settings"]["ratio"]
    p, N = c["p"], 5
    m = model(rl, c)
    truth = {3: [p - 1, p - 2, 20], 9: [p - 3, 30], 7: [5]}  # high ids: first in no sorted list
    m.compute_recommendation(alpha=s["alpha"], lam_bda=s["lam"], max_iter=s["max_iter"], tol=s["tol"],
                             N=N, ground_truth=truth, val_ur=truth, lambda_is_ratio=True)
    assert not m.score_rows([3, 9]).any()
    for rec in (m.recommendation, m.val_recommendation):
        assert rec[3] == [0, 1, 2, 3, 4]  # all 48 items are candidates, all tie at 0
        assert rec[9] == [0, 1, 2, 3, 4]  # every item but the train item 11
        assert not set(rec[3]) & set(truth[3]) and not set(rec[9]) & set(truth[9])
        assert rec[7] == [5, 11]  # user 7 trained on every other item; both score 0
    # the lists themselves: ascending ids, whatever the truth is
    off, items = m._candidates(lambda u: truth.get(u, []), np.random.default_rng(0))
    for u in range(c["U"]):
        lst = items[off[u]:off[u + 1]]
        assert (np.diff(lst) > 0).all(), u
    m.close()


def test_compute_recommendation_has_the_reference_entry(rl):
    c, s = CASES["s60"], CASES["s60"]["settings"]["ratio"]

    class Data:
        train = [c["pairs"].tolist()]
        num_user, num_item = c["U"], c["p"]

    m = rl.SLIM(Data, 0)
    truth = {u: [int(x) for x in np.flatnonzero(S.dense(c["pairs"], c["U"], c["p"])[u] == 0)[:3]]
             for u in range(0, c["U"], 2)}
    m.compute_recommendation(alpha=s["alpha"], lam_bda=s["lam"], max_iter=s["max_iter"], tol=s["tol"],
                             N=5, ground_truth=truth, val_ur={}, lambda_is_ratio=True)
    assert same_bits(m.W, s["W"])
    assert len(m.recommendation) == len(m.val_recommendation) == c["U"]
    A = S.dense(c["pairs"], c["U"], c["p"])
    AW = S.score_rows(*c["csr"], s["W"], np.arange(c["U"]))
    for u, rec in enumerate(m.recommendation):
        assert len(rec) == len(set(rec)) <= 5
        assert all(A[u, i] == 0 for i in rec)  # candidates exclude the train items
        cand = sorted(set(range(c["p"])) - set(np.flatnonzero(A[u]).tolist()))
        if len(cand) >= 5:  # fewer than 1000 candidates exist: every one of them is in the list
            assert len(rec) == 5
            assert sorted(AW[u, rec], reverse=True) == sorted(AW[u, cand], reverse=True)[:5]
    m.close()


# ---- 5. errors ---------------------------------------------------------------------------------
def test_call_order_is_checked(rl):
    import ctypes
    L = rl._lib.load()
    cfg = rl.slim.SlimConfig(user_num=4, item_num=3, device=0, chip_max_p=0)
    h = ctypes.c_void_p()
    assert L.slim_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    st = rl.slim.SlimStats()
    E_STATE, E_RANGE, E_INVALID = rl._lib.E_STATE, rl._lib.E_RANGE, rl._lib.E_INVALID
    assert L.slim_gram(h, None) == E_STATE
    assert L.slim_fit(h, 0.5, 0.02, 1, 10, 1e-4, 0, 3, ctypes.byref(st)) == E_STATE
    sec = ctypes.c_double(-1.0)
    assert L.slim_gram_seconds(h, ctypes.byref(sec)) == E_STATE
    u = np.array([0, 1, 1, 3], np.int32)
    i = np.array([0, 2, 2, 1], np.int32)
    bad_i, bad_u, neg = np.array([0, 3, 2, 1], np.int32), u + 1, np.array([0, -1, 2, 1], np.int32)
    assert L.slim_set_train(h, u.ctypes.data, bad_i.ctypes.data, 4) == E_RANGE
    assert L.slim_set_train(h, bad_u.ctypes.data, i.ctypes.data, 4) == E_RANGE
    assert L.slim_set_train(h, u.ctypes.data, neg.ctypes.data, 4) == E_RANGE
    assert L.slim_gram(h, None) == E_STATE  # a rejected train set is no train set
    assert L.slim_set_train(h, u.ctypes.data, i.ctypes.data, 4) == 0
    assert L.slim_fit(h, 0.5, 0.02, 1, 10, 1e-4, 0, 3, ctypes.byref(st)) == E_STATE
    assert b"slim_gram" in L.bprmf_last_error()
    out = np.empty(1)
    assert L.slim_score(h, u.ctypes.data, i.ctypes.data, 1, out.ctypes.data) == E_STATE
    assert L.slim_gram(h, None) == 0
    assert L.slim_gram_seconds(h, ctypes.byref(sec)) == 0 and sec.value > 0
    assert L.slim_gram_seconds(h, None) == E_INVALID
    assert L.slim_fit(h, 0.5, 0.02, 1, 10, 1e-4, 0, 3, ctypes.byref(st)) == 0
    assert st.columns == 3 and st.gram_seconds == sec.value
    for args in [(-0.1, 0.02, 1, 10, 1e-4), (1.1, 0.02, 1, 10, 1e-4), (float("nan"), 0.02, 1, 10, 1e-4),
                 (0.5, -1.0, 1, 10, 1e-4), (0.5, 0.02, 1, -1, 1e-4), (0.5, 0.02, 1, 10, -1e-4),
                 (0.0, 0.02, 1, 10, 1e-4)]:
        assert L.slim_fit(h, *args, 0, 3, ctypes.byref(st)) == E_INVALID, args
    assert L.slim_fit(h, 0.0, 0.02, 0, 10, 1e-4, 0, 3, ctypes.byref(st)) == 0  # alpha 0, absolute
    assert L.slim_fit(h, 0.5, 0.02, 1, 10, 1e-4, 2, 4, ctypes.byref(st)) == E_INVALID
    assert L.slim_fit(h, 0.5, 0.02, 1, 10, 1e-4, 2, 1, ctypes.byref(st)) == E_INVALID
    pos, sc = np.empty(40, np.int32), np.empty(40)
    off = np.array([0, 2], np.int64)
    for k in (0, 33):
        assert L.slim_topk_lists(h, u.ctypes.data, off.ctypes.data, i.ctypes.data, 1, k,
                                 pos.ctypes.data, sc.ctypes.data) == E_INVALID
    four, i2, row = np.array([4], np.int32), i + 2, np.empty(3)
    assert L.slim_score(h, four.ctypes.data, i.ctypes.data, 1, out.ctypes.data) == E_RANGE
    assert L.slim_score_rows(h, four.ctypes.data, 1, row.ctypes.data) == E_RANGE
    assert L.slim_topk_lists(h, four.ctypes.data, off.ctypes.data, i.ctypes.data, 1, 2,
                             pos.ctypes.data, sc.ctypes.data) == E_RANGE
    assert L.slim_topk_lists(h, u.ctypes.data, off.ctypes.data, i2.ctypes.data, 1, 2,
                             pos.ctypes.data, sc.ctypes.data) == E_RANGE
    assert L.slim_destroy(h) == 0


def test_gram_refuses_a_catalogue_that_does_not_fit(rl):
    p = 300_000  # G and W would be 1.44 TB; the operand (300,032 x 128 bytes) is small
    m = rl.SLIM(np.array([[0, 0], [0, p - 1]]), num_user=1, num_item=p)
    with pytest.raises(rl.BprmfError, match=r"G and W .* needs 1440\.\d+ GB of device memory"):
        m.gram(fetch=False)
    with pytest.raises(rl.BprmfError, match="device memory"):  # fit() asks for the Gram matrix again
        m.fit()
    m.close()


def test_python_argument_errors(rl):
    pairs = np.array([[0, 0], [1, 2], [3, 1]])
    with pytest.raises(ValueError):
        rl.SLIM(pairs)  # sizes missing
    with pytest.raises(IndexError):
        rl.SLIM(pairs, num_user=3, num_item=3)
    with pytest.raises(IndexError):
        rl.SLIM(pairs, num_user=4, num_item=2)
    with pytest.raises(ValueError):
        rl.SLIM(pairs.ravel(), num_user=4, num_item=3)
    m = rl.SLIM(pairs, num_user=4, num_item=3)
    assert m.W is None
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(lam_bda=-1), dict(tol=-1), dict(max_iter=-1),
               dict(alpha=0.0, lambda_is_ratio=True), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            m.fit(**kw)
    with pytest.raises(IndexError):
        m.fit(columns=(0, 4))
    m.fit(alpha=0.0, lambda_is_ratio=False)
    assert m.W.shape == (3, 3)
    with pytest.raises(IndexError):
        m.predict_batch([4], [0])
    with pytest.raises(IndexError):
        m.predict(0, 3)
    with pytest.raises(IndexError):
        m.score_rows([-1])
    with pytest.raises(ValueError):
        m.predict_batch([0, 1], [0])
    with pytest.raises(ValueError):
        m.recommend([0], [0, 1], [0], N=33)
    with pytest.raises(ValueError):
        m.recommend([0], [0], [0])
    with pytest.raises(ValueError):
        m.recommend([0], [0, 2], [0])
    with pytest.raises(IndexError):
        m.recommend([0], [0, 1], [3])
    m.close()
