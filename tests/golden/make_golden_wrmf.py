"""Generate the WRMF fixtures by IMPORTING the reference's model class (WRMFRecommender.WRMF,
WRMFRecommender.py:24-62) in the build container and running its fit().  The reference is not
copied; only its inputs and outputs are written.

Cases (U, I, d, density, epochs; numpy seed): ratings are integers 1..5, seed=2019, alpha=40,
lambda_val=0.1.  Every case has an empty user (row 3), an empty item (column 5), a user with
every other item (row 7) and a user with one interaction (row 9, item 11).
wrmf_cases.npz, per case c: c_shape [U, I, d, epochs], the ratings' CSR (c_indptr, c_indices,
c_data), c_X0 / c_Y0 (the constructor's draws), c_X / c_Y (after fit()), and c_dist_X / c_dist_Y =
max|reference - restatement| / max|reference| for tests/wrmf_numpy.py in reference mode.
Run:  python tests/golden/make_golden_wrmf.py
"""
import os
import sys
import warnings

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
CASES = [("c8", 40, 60, 8, 0.15, 3, 1), ("c20", 70, 50, 20, 0.10, 3, 2),
         ("c32", 48, 96, 32, 0.20, 2, 3), ("c128", 33, 47, 128, 0.20, 2, 4)]
ALPHA, LAMBDA, SEED = 40, 0.1, 2019


def ratings(U, I, density, seed):
    g = np.random.default_rng(seed)
    R = np.where(g.random((U, I)) < density, g.integers(1, 6, (U, I)), 0).astype(np.float64)
    R[7, :] = 0
    R[7, 0::2] = g.integers(1, 6, len(R[7, 0::2]))
    R[9, :] = 0
    R[9, 11] = 4
    R[3, :] = 0
    R[:, 5] = 0
    return R


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(OUT))
    import scipy.sparse as sp
    from WRMFRecommender import WRMF  # the reference model (:24-62)
    import wrmf_numpy as W

    out = {}
    for name, U, I, d, density, epochs, seed in CASES:
        csr = sp.csr_matrix(ratings(U, I, density, seed))
        assert csr[3].nnz == 0 and csr[:, 5].nnz == 0 and csr[9].nnz == 1 and csr[7].nnz == (I + 1) // 2
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # SparseEfficiencyWarning of the reference's row writes
            m = WRMF(csr, lambda_val=LAMBDA, alpha=ALPHA, iterations=epochs, factor_num=d, seed=SEED)
            X0, Y0 = m.X.toarray(), m.Y.toarray()
            m.fit()
        X, Y = m.X.toarray(), m.Y.toarray()
        indptr, indices, data, _ = W.as_csr(csr)
        Xn, Yn = W.fit((indptr, indices, ALPHA * data, (U, I)), X0, Y0, LAMBDA, epochs)
        dist = [np.abs(a - b).max() / np.abs(a).max() for a, b in ((X, Xn), (Y, Yn))]
        print(name, "dist_X %.3e dist_Y %.3e max|X| %.3g" % (dist[0], dist[1], np.abs(X).max()),
              file=sys.stderr)
        c = dict(shape=np.array([U, I, d, epochs]), indptr=indptr, indices=indices, data=data,
                 X0=X0, Y0=Y0, X=X, Y=Y, dist_X=dist[0], dist_Y=dist[1])
        for k, v in c.items():
            out[f"{name}_{k}"] = np.asarray(v)
    out["cases"] = np.array([c[0] for c in CASES])
    np.savez_compressed(os.path.join(OUT, "wrmf_cases.npz"), **out)


if __name__ == "__main__":
    main()
