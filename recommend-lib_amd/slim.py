"""SLIM — drop-in for the reference's item-item elastic net (SLiMRecommender.py:27-149 with
util/slim.pyx).

`SLIM(data, i)` takes what the reference's constructor takes (an object with `.train[i]`,
`.num_user`, `.num_item`, as util.data_loader.SlimData has) or an [n, 2] array of (user, item)
pairs with `num_user=` and `num_item=`.  `compute_recommendation(...)` has the reference's
signature and fills `W`, `recommendation` and `val_recommendation`; `fit(...)` is the training
alone.  A[u, i] = 1 for every pair (duplicates collapse), G = A^T A is computed exactly on i8
MFMA, and every column of W is the reference's coordinate descent in f64 with the reference's
operation order: W equals the compiled reference bit for bit (include/slim.h, slim.hip).

compute_recommendation draws each user's 1000 candidates (:104-111) on the host from
numpy.random.default_rng(seed); it does NOT reproduce the reference's `random.sample` over a set,
whose order depends on the interpreter.  Every candidate list is in ascending item id, whether an
item is ground truth or sampled, and among equal scores the earlier candidate ranks first (as the
reference's `sorted(..., reverse=True)` does on its list): ties, of which a sparse W gives many at
exactly 0, go to the smaller item id and never to the truth as such.
"""
import ctypes

import numpy as np

from . import _lib

TOPK_MAX = 32  # SLIM_TOPK_MAX


class SlimConfig(ctypes.Structure):  # slim_config, include/slim.h
    _fields_ = [("user_num", ctypes.c_int64), ("item_num", ctypes.c_int64),
                ("device", ctypes.c_int32), ("chip_max_p", ctypes.c_int32)]


class SlimStats(ctypes.Structure):  # slim_stats
    _fields_ = [("columns", ctypes.c_int64), ("sweeps", ctypes.c_int64), ("moves", ctypes.c_int64),
                ("capped", ctypes.c_int64), ("gram_seconds", ctypes.c_double),
                ("cd_seconds", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _ids(a, what):
    a = np.asarray(a)
    if a.ndim != 1:
        raise ValueError(f"{what} must be 1-d")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must be integers")
    return np.ascontiguousarray(a, np.int32) if a.size else np.zeros(0, np.int32)


class SLIM(_lib.Handle):
    """SLiMRecommender.py:27-149 on the GPU."""

    def __init__(self, data, i=None, *, num_user=None, num_item=None, device=0, chip_max_p=0):
        if hasattr(data, "train"):
            pairs = data.train if i is None else data.train[i]
            num_user = data.num_user if num_user is None else num_user
            num_item = data.num_item if num_item is None else num_item
        else:
            pairs = data
        if num_user is None or num_item is None:
            raise ValueError("an array of pairs needs num_user= and num_item=")
        pairs = np.asarray(pairs)
        if pairs.size == 0:
            pairs = np.zeros((0, 2), np.int64)
        if pairs.ndim != 2 or pairs.shape[1] != 2:
            raise ValueError("pairs must be [n, 2] (user, item) rows")
        if not np.issubdtype(pairs.dtype, np.integer):
            raise ValueError("pairs must be integers")
        if num_user < 0 or num_item < 0 or chip_max_p < 0:
            raise ValueError("num_user, num_item and chip_max_p must be >= 0")
        self.data, self.i = data, i
        self.num_user, self.num_item = int(num_user), int(num_item)
        if len(pairs) and (pairs.min() < 0 or pairs[:, 0].max() >= self.num_user
                           or pairs[:, 1].max() >= self.num_item):
            raise IndexError("user or item id out of range")
        self.alpha = self.lam_bda = self.max_iter = self.tol = self.N = self.lambda_is_ratio = None
        self.recommendation = self.val_recommendation = None
        self.last_stats = None
        self._W = None
        self._have_gram = False
        cfg = SlimConfig(user_num=self.num_user, item_num=self.num_item, device=int(device),
                         chip_max_p=int(chip_max_p))
        self._open("slim", cfg)
        u = np.ascontiguousarray(pairs[:, 0], np.int32)
        it = np.ascontiguousarray(pairs[:, 1], np.int32)
        _lib.check(self._L.slim_set_train(self._h, _lib.ptr(u), _lib.ptr(it), len(u)))
        # the users' train items, ascending (compute_recommendation's exclusion sets)
        key = np.unique(pairs[:, 0].astype(np.int64) * max(self.num_item, 1) + pairs[:, 1])
        self._train_user = key // max(self.num_item, 1)
        self._train_item = key % max(self.num_item, 1)

    # ---- training ------------------------------------------------------------------------------
    def gram(self, fetch=True):
        """G = A^T A [p, p], exact; kept on the device for fit().  fetch=False returns the device
        seconds instead of copying G back."""
        p = self.num_item
        G = np.empty((p, p)) if fetch else None
        _lib.check(self._L.slim_gram(self._h, _lib.ptr(G)))
        self._have_gram, self._W = True, None
        if fetch:
            return G
        seconds = ctypes.c_double()
        _lib.check(self._L.slim_gram_seconds(self._h, ctypes.byref(seconds)))
        return seconds.value

    def fit(self, alpha=0.5, lam_bda=0.02, max_iter=1000, tol=1e-4, lambda_is_ratio=True, columns=None):
        """The reference's __aggregation_coefficients (:48-91).  columns=(begin, end) fits that
        range of W's columns and leaves the others as they are."""
        alpha, lam_bda, tol = float(alpha), float(lam_bda), float(tol)
        if not (lam_bda >= 0 and tol >= 0 and int(max_iter) >= 0 and np.isfinite(lam_bda) and np.isfinite(tol)):
            raise ValueError("need finite lam_bda >= 0, tol >= 0 and max_iter >= 0")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("alpha must be in [0, 1]")
        if lambda_is_ratio and alpha == 0.0:
            raise ValueError("alpha == 0 with lambda_is_ratio divides by zero")
        begin, end = (0, self.num_item) if columns is None else (int(columns[0]), int(columns[1]))
        if not 0 <= begin <= end <= self.num_item:
            raise IndexError("columns out of range")
        if not self._have_gram:
            self.gram(fetch=False)
        self.alpha, self.lam_bda, self.max_iter, self.tol = alpha, lam_bda, int(max_iter), tol
        self.lambda_is_ratio = bool(lambda_is_ratio)
        st = SlimStats()
        _lib.check(self._L.slim_fit(self._h, alpha, lam_bda, int(bool(lambda_is_ratio)), int(max_iter),
                                    tol, begin, end, ctypes.byref(st)))
        self.last_stats = st.as_dict()
        self._W = None
        return self

    def weights(self, columns=None):
        """W[:, begin:end] as a dense float64 array."""
        begin, end = (0, self.num_item) if columns is None else (int(columns[0]), int(columns[1]))
        if not 0 <= begin <= end <= self.num_item:
            raise IndexError("columns out of range")
        out = np.empty((self.num_item, end - begin))
        _lib.check(self._L.slim_get_weights(self._h, begin, end, _lib.ptr(out)))
        return out

    @property
    def W(self):
        """The dense [p, p] array the reference exposes (:143); None before gram() / fit()."""
        if self._W is None and self._have_gram:
            self._W = self.weights()
        return self._W

    # ---- scores --------------------------------------------------------------------------------
    def predict_batch(self, users, items):
        """(A W)[u, i] per pair: the user's W[j, i] added in ascending j."""
        u, i = _ids(users, "users"), _ids(items, "items")
        if u.shape != i.shape:
            raise ValueError("users and items must be 1-d arrays of one length")
        if len(u) and (u.min() < 0 or u.max() >= self.num_user or i.min() < 0 or i.max() >= self.num_item):
            raise IndexError("user or item id out of range")
        out = np.empty(len(u), np.float64)
        _lib.check(self._L.slim_score(self._h, _lib.ptr(u), _lib.ptr(i), len(u), _lib.ptr(out)))
        return out

    def predict(self, u, i):
        if not (0 <= u < self.num_user and 0 <= i < self.num_item):
            raise IndexError("user or item id out of range")
        return float(self.predict_batch([u], [i])[0])

    def score_rows(self, users):
        """Rows of A W (:123) for the given users: [n, p]."""
        u = _ids(users, "users")
        if len(u) and (u.min() < 0 or u.max() >= self.num_user):
            raise IndexError("user id out of range")
        out = np.empty((len(u), self.num_item), np.float64)
        _lib.check(self._L.slim_score_rows(self._h, _lib.ptr(u), len(u), _lib.ptr(out)))
        return out

    def recommend(self, users, offsets, items, N=10):
        """Per user r the N best of items[offsets[r]:offsets[r + 1]]: (positions [n, N] within the
        user's list, scores [n, N]); score descending, ties by the earlier position; -1 and -inf
        past a list's end."""
        u, it = _ids(users, "users"), _ids(items, "items")
        off = np.ascontiguousarray(offsets, np.int64)
        if off.ndim != 1 or len(off) != len(u) + 1:
            raise ValueError("offsets must hold len(users) + 1 entries")
        if not 1 <= int(N) <= TOPK_MAX:
            raise ValueError(f"N must be in 1..{TOPK_MAX}")
        if off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > len(it):
            raise ValueError("offsets must start at >= 0, not decrease and end within items")
        if (len(u) and (u.min() < 0 or u.max() >= self.num_user)) or \
                (len(it) and (it.min() < 0 or it.max() >= self.num_item)):
            raise IndexError("user or item id out of range")
        pos = np.empty((len(u), int(N)), np.int32)
        score = np.empty((len(u), int(N)), np.float64)
        _lib.check(self._L.slim_topk_lists(self._h, _lib.ptr(u), _lib.ptr(off), _lib.ptr(it), len(u),
                                           int(N), _lib.ptr(pos), _lib.ptr(score)))
        return pos, score

    # ---- the reference's driver entry (:130-149) -------------------------------------------------
    def _candidates(self, truth_of, rng, max_i_num=1000):
        """(offsets, items): per user the candidate set of :104-111 in ascending item id, so a
        list's order says nothing about which of its items are the truth (the reference ranks
        `set(candidates)`, :114, whose order for small ints is close to ascending too)."""
        lists = []
        starts = np.searchsorted(self._train_user, np.arange(self.num_user + 1))
        for u in range(self.num_user):
            truth = np.asarray(list(dict.fromkeys(truth_of(u))), np.int64)
            if len(truth) < max_i_num:
                seen = np.zeros(self.num_item, bool)
                seen[self._train_item[starts[u]:starts[u + 1]]] = True
                seen[truth] = True
                pool = np.flatnonzero(~seen)
                take = min(max_i_num - len(truth), len(pool))
                lists.append(np.sort(np.concatenate([truth, rng.choice(pool, take, replace=False)])))
            else:
                lists.append(np.sort(rng.choice(truth, max_i_num, replace=False)))
        offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        items = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
        return offsets, items

    def _get_recommendation(self, truth, rng):
        get = (lambda u: truth.get(u, [])) if hasattr(truth, "get") else (lambda u: truth[u])
        offsets, items = self._candidates(get, rng)
        users = np.arange(self.num_user, dtype=np.int32)
        pos, _ = self.recommend(users, offsets, items, self.N)
        return [[int(items[offsets[u] + q]) for q in pos[u] if q >= 0] for u in range(self.num_user)]

    def compute_recommendation(self, alpha=0.5, lam_bda=0.02, max_iter=1000, tol=0.0001, N=10,
                               ground_truth=None, val_ur=None, lambda_is_ratio=True, seed=0):
        self.N = N
        self.ur, self.val_ur = ground_truth, val_ur
        self.fit(alpha, lam_bda, max_iter, tol, lambda_is_ratio)
        rng = np.random.default_rng(seed)
        self.val_recommendation = self._get_recommendation({} if val_ur is None else val_ur, rng)
        self.recommendation = self._get_recommendation({} if ground_truth is None else ground_truth, rng)
