"""Generate the SLIM fixtures by COMPILING AND CALLING the reference's util/slim.pyx (cythonize into
a temporary directory outside this repository) the way SLiMRecommender.py:48-91 drives it: blocks
of 100 columns (so start > 0 is covered), compute_covariance + symmetrize_covariance, then
coordinate_descent / coordinate_descent_lambda_ratio, then A.dot(W) (:123).  The reference is not
copied; only its inputs and outputs are written.  At generation time the restatement
(tests/slim_numpy.py) must equal the reference's W bit for bit, or nothing is written.

Cases (U x p, density, seed) and their settings (alpha, lam_bda, max_iter, tol, lambda_is_ratio):
  s60   60 x  48  ratio and absolute
  s200  200 x 130 ratio and absolute, alpha = 1 (c = 0, so 0/0 at the unrated item) and
                  max_iter = 5 (the cap reached mid-alternation)
  s700  700 x 530 ratio (more than two scan blocks of a 256-thread workgroup)
Every A has an item nobody rated (5), two identical item columns (8 = 2), an item (11) whose only
user (9) rated nothing else (max_cov == 0), an empty user (3) and a user (7) with every item but
5 and 11, which have to stay unrated / isolated.
slim_cases.npz, per case c: c_shape [U, p], c_pairs [n, 2] (with some duplicate rows), c_aw_users
(the rows of A.W that are stored: all of them, or a sample that holds users 3, 7 and 9), and per
setting s: c_s_setting [alpha, lam_bda, max_iter, tol, ratio], c_s_w_idx / c_s_w_val (W's
non-zeros: flat row-major indices and values), c_s_aw [len(aw_users), p], c_s_counters [p, 3]
(the restatement's sweeps, moves, capped per column).
Run:  python tests/golden/make_golden_slim.py --ref <reference checkout>  [--time]
--time runs the reference, single process, on the matrix of tools/bench_slim.py --shape ml-100k
and writes the seconds to profiles/slim_reference_cpu.json.
"""
import argparse
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
GROUP = 100  # SLiMRecommender.py:49
DEFAULT = (0.5, 0.02, 1000, 1e-4)  # SLiMRecommender.py:130
CASES = [
    ("s60", 60, 48, 0.15, 1, 0, {"ratio": DEFAULT + (1,), "abs": DEFAULT + (0,)}),
    ("s200", 200, 130, 0.10, 2, 50, {"ratio": DEFAULT + (1,), "abs": DEFAULT + (0,),
                                     "lasso": (1.0, 0.02, 1000, 1e-4, 1),
                                     "cap5": (0.5, 0.02, 5, 1e-4, 1)}),
    ("s700", 700, 530, 0.06, 3, 64, {"ratio": DEFAULT + (1,)}),
]


def pairs_of(U, p, density, seed):
    g = np.random.default_rng(seed)
    pop = 1.0 / np.sqrt(1.0 + g.permutation(p))  # popularity skew
    A = g.random((U, p)) < density * pop / pop.mean()
    A[:, 8] = A[:, 2]
    A[7, :] = True
    A[3, :] = False
    A[9, :] = False
    A[:, 5] = False
    A[:, 11] = False
    A[9, 11] = True
    u, i = np.nonzero(A)
    pairs = np.stack([u, i], axis=1).astype(np.int64)
    pairs = np.concatenate([pairs, pairs[:: max(1, len(pairs) // 7)]])  # duplicates collapse
    return pairs[g.permutation(len(pairs))]


def build_reference(ref):
    """util/slim.pyx compiled in a temporary directory; returns (module, directory)."""
    tmp = tempfile.mkdtemp(prefix="slim_ref_")
    shutil.copy(os.path.join(ref, "util", "slim.pyx"), tmp)
    env = dict(os.environ, CFLAGS=f"-O2 -ffp-contract=off -w -I{np.get_include()}")
    # cdivision: with Cython's default (Python division) the reference raises ZeroDivisionError at
    # the 0/0 of an unrated item under c == 0 (the "lasso" setting); C division gives the NaN that
    # its `abs_double(delta) > tol` then treats as no move.  Every other result is the same.
    subprocess.run([sys.executable, "-m", "cython", "-3", "-X", "cdivision=True", "slim.pyx"], cwd=tmp, check=True, env=env)
    import sysconfig
    so = "slim" + sysconfig.get_config_var("EXT_SUFFIX")
    subprocess.run(["gcc", "-shared", "-fPIC", *env["CFLAGS"].split(),
                    "-I" + sysconfig.get_paths()["include"], "slim.c", "-o", so], cwd=tmp, check=True)
    sys.path.insert(0, tmp)
    return importlib.import_module("slim"), tmp


def blocks(p):
    return [(s, min(p, s + GROUP)) for s in range(0, p, GROUP)]


def reference_gram(slim, A):
    G = np.vstack([slim.compute_covariance(A, s, e) for s, e in blocks(A.shape[1])])
    slim.symmetrize_covariance(G)
    return G


def reference_fit(slim, G, U, setting):
    alpha, lam, max_iter, tol, ratio = setting
    cd = slim.coordinate_descent_lambda_ratio if ratio else slim.coordinate_descent
    p = G.shape[0]
    return np.hstack([cd(alpha, lam, int(max_iter), tol, U, p, G, s, e) for s, e in blocks(p)])


def make_cases(slim):
    sys.path.insert(0, os.path.dirname(OUT))
    import slim_numpy as S

    out = {}
    for name, U, p, density, seed, n_aw, settings in CASES:
        pairs = pairs_of(U, p, density, seed)
        A = S.dense(pairs, U, p)
        assert not A[:, 5].any() and not A[3].any() and A[9].sum() == 1 and A[:, 11].sum() == 1
        assert np.array_equal(A[:, 8], A[:, 2]) and A[7].sum() == p - 2
        assert U % 32 and p % 32
        G = reference_gram(slim, A)
        assert np.array_equal(G, S.gram(pairs, U, p))
        if n_aw:
            aw_users = np.unique(np.concatenate([[3, 7, 9], np.arange(0, U, U // n_aw)]))
        else:
            aw_users = np.arange(U)
        out[f"{name}_shape"] = np.array([U, p])
        out[f"{name}_pairs"] = pairs.astype(np.int32)
        out[f"{name}_aw_users"] = aw_users.astype(np.int32)
        for tag, setting in settings.items():
            W = reference_fit(slim, G, U, setting)
            alpha, lam, max_iter, tol, ratio = setting
            Wn, counters = S.fit(G, alpha, lam, bool(ratio), int(max_iter), tol, U)
            assert np.array_equal(W.view(np.int64), Wn.view(np.int64)), (name, tag)
            AW = A.dot(W)
            idx = np.flatnonzero(W)
            print(name, tag, "nnz(W)", len(idx), "sweeps/moves/capped", counters.sum(0), file=sys.stderr)
            k = f"{name}_{tag}"
            out[k + "_setting"] = np.array(setting, np.float64)
            out[k + "_w_idx"] = idx.astype(np.int32)
            out[k + "_w_val"] = W.ravel()[idx]
            out[k + "_aw"] = AW[aw_users]
            out[k + "_counters"] = counters.astype(np.int32)
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(OUT, "slim_cases.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)


def time_reference(slim):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.dirname(OUT))
    import bench_slim as B
    import slim_numpy as S

    U, p, _ = B.SHAPES["ml-100k"]
    pairs = B.train_pairs("ml-100k")
    A = S.dense(pairs, U, p)
    t0 = time.perf_counter()
    G = reference_gram(slim, A)
    t_gram = time.perf_counter() - t0
    res = {"what": "util/slim.pyx, one process, the matrix of tools/bench_slim.py --shape ml-100k",
           "shape": [U, p], "pairs": int(A.sum()), "gram_seconds": round(t_gram, 3)}
    for tag, ratio in (("cd_ratio_seconds", 1), ("cd_abs_seconds", 0)):
        t0 = time.perf_counter()
        W = reference_fit(slim, G, U, DEFAULT + (ratio,))
        res[tag] = round(time.perf_counter() - t0, 3)
        res[tag.replace("seconds", "nnz")] = int(np.count_nonzero(W))
    res["setting"] = dict(alpha=DEFAULT[0], lam_bda=DEFAULT[1], max_iter=DEFAULT[2], tol=DEFAULT[3])
    with open(os.path.join(ROOT, "profiles", "slim_reference_cpu.json"), "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REFERENCE_DIR"), help="the reference checkout")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if not a.ref:
        ap.error("--ref (or REFERENCE_DIR) is needed")
    sys.dont_write_bytecode = True
    slim, tmp = build_reference(a.ref)
    try:
        time_reference(slim) if a.time else make_cases(slim)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
