"""WRMF — drop-in for the reference's implicit-feedback ALS model (WRMFRecommender.py:24-62).

The same constructor arguments, `fit()`, `predict(u, i)` and the `user_vec` / `item_vec`
attributes the reference's driver reads (:147, :179).  The constructor draws X then Y from
np.random.RandomState(seed) exactly as the reference does (:27-32), so the same seed gives the
same start; the epochs run on the GPU in double (include/wrmf.h, wrmf.hip).

gram="reference" (default) keeps the reference's epoch: both Gram matrices are taken before the
user sweep (:39-40), so the item sweep solves against the XtX of the old X.  gram="fresh"
recomputes XtX after the user sweep (textbook ALS).  predict() returns the float the reference's
`.A[0, 0]` was meant to return (that line fails with current SciPy).
"""
import ctypes

import numpy as np

from . import _lib


class WrmfConfig(ctypes.Structure):  # wrmf_config, include/wrmf.h
    _fields_ = [("user_num", ctypes.c_int64), ("item_num", ctypes.c_int64),
                ("factor_num", ctypes.c_int32), ("device", ctypes.c_int32),
                ("lambda_val", ctypes.c_double), ("gram_mode", ctypes.c_int32),
                ("heavy_nnz", ctypes.c_int32)]


class WrmfStats(ctypes.Structure):  # wrmf_stats
    _fields_ = [("solves", ctypes.c_int64), ("heavy_rows", ctypes.c_int64),
                ("seconds", ctypes.c_double)]

    def as_dict(self):
        return dict(solves=self.solves, heavy_rows=self.heavy_rows, seconds=self.seconds)


GRAM_MODES = {"reference": 0, "fresh": 1}


def _csr(train_set):
    """(indptr int64, indices int32, data float64, (U, I)) of a SciPy sparse matrix or such a
    tuple; a SciPy matrix gets its duplicates summed and its column indices sorted."""
    if isinstance(train_set, tuple):
        indptr, indices, data, shape = train_set
    else:
        import scipy.sparse as sp  # lazy: only this entry point needs SciPy

        m = sp.csr_matrix(train_set, copy=True)
        m.sum_duplicates()
        m.sort_indices()
        indptr, indices, data, shape = m.indptr, m.indices, m.data, m.shape
    return (np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32),
            np.ascontiguousarray(data, np.float64), (int(shape[0]), int(shape[1])))


class WRMF(_lib.Handle):
    """WRMFRecommender.py:24-62 on the GPU."""

    def __init__(self, train_set, lambda_val=0.1, alpha=40, iterations=10, factor_num=20, seed=2019,
                 *, gram="reference", device=0, heavy_nnz=0):
        if gram not in GRAM_MODES:
            raise ValueError(f"gram must be one of {sorted(GRAM_MODES)}")
        self.epochs = iterations
        self.lambda_val, self.alpha, self.factor_num, self.gram_mode = lambda_val, alpha, factor_num, gram
        indptr, indices, data, (U, I) = _csr(train_set)
        self.num_user, self.num_item = U, I
        self.rstate, self._X, self._Y = self.initial_factors(U, I, factor_num, seed)
        self.last_stats = None
        cfg = WrmfConfig(user_num=U, item_num=I, factor_num=int(factor_num), device=int(device),
                         lambda_val=float(lambda_val), gram_mode=GRAM_MODES[gram],
                         heavy_nnz=int(heavy_nnz))
        self._open("wrmf", cfg)
        conf = np.ascontiguousarray(alpha * data, np.float64)  # :28 C = alpha * train_set
        _lib.check(self._L.wrmf_set_train(self._h, _lib.ptr(indptr), _lib.ptr(indices),
                                          _lib.ptr(conf), len(indices)))
        self._push()

    @staticmethod
    def initial_factors(num_user, num_item, factor_num, seed=2019):
        """(rstate, X0, Y0) as the reference's constructor draws them (:27, :31-32): users first."""
        rstate = np.random.RandomState(seed)
        X = rstate.normal(scale=0.01, size=(num_user, factor_num))
        Y = rstate.normal(scale=0.01, size=(num_item, factor_num))
        return rstate, X, Y

    def _push(self):
        _lib.check(self._L.wrmf_set_weights(self._h, _lib.ptr(self._X), _lib.ptr(self._Y)))

    def _pull(self):
        X = np.empty((self.num_user, self.factor_num))
        Y = np.empty((self.num_item, self.factor_num))
        _lib.check(self._L.wrmf_get_weights(self._h, _lib.ptr(X), _lib.ptr(Y)))
        self._X, self._Y = X, Y

    def set_factors(self, X, Y):
        X = np.ascontiguousarray(X, np.float64)
        Y = np.ascontiguousarray(Y, np.float64)
        if X.shape != (self.num_user, self.factor_num) or Y.shape != (self.num_item, self.factor_num):
            raise ValueError("X must be [num_user, factor_num] and Y [num_item, factor_num]")
        self._X, self._Y = X.copy(), Y.copy()
        self._push()

    def factors(self):
        """(X [U, d], Y [I, d]) as dense float64 arrays."""
        return self._X.copy(), self._Y.copy()

    def gram(self, side):
        """G = XtX (side 0) or YtY (side 1) of the device's tables; stored for the next sweep."""
        G = np.empty((self.factor_num, self.factor_num))
        _lib.check(self._L.wrmf_gram(self._h, int(side), _lib.ptr(G)))
        return G

    def sweep(self, side):
        """Solve every user row (side 0) or item row (side 1) against the stored Gram matrix."""
        st = WrmfStats()
        _lib.check(self._L.wrmf_sweep(self._h, int(side), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        self._pull()
        return self.last_stats

    def fit(self, epochs=None):
        import scipy.sparse as sp

        st = WrmfStats()
        n = self.epochs if epochs is None else epochs
        _lib.check(self._L.wrmf_fit(self._h, int(n), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        self._pull()
        # :58, what the reference's driver multiplies (:147, :179)
        self.user_vec, self.item_vec = sp.csr_matrix(self._X), sp.csr_matrix(self._Y).T.tocsr()
        return self

    def predict_batch(self, users, items):
        u = np.ascontiguousarray(users, np.int32)
        i = np.ascontiguousarray(items, np.int32)
        if u.shape != i.shape or u.ndim != 1:
            raise ValueError("users and items must be 1-d arrays of one length")
        if len(u) and (u.min() < 0 or u.max() >= self.num_user or i.min() < 0 or i.max() >= self.num_item):
            raise IndexError("user or item id out of range")
        out = np.empty(len(u), np.float64)
        _lib.check(self._L.wrmf_predict(self._h, _lib.ptr(u), _lib.ptr(i), len(u), _lib.ptr(out)))
        return out

    def predict(self, u, i):
        if not (0 <= u < self.num_user and 0 <= i < self.num_item):
            raise IndexError("user or item id out of range")
        return float(self.predict_batch([u], [i])[0])
