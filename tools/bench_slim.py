"""Measurement of SLIM (SLiMRecommender.py:48-91): the Gram matrix on i8 MFMA and the coordinate
descent of every column on the GPU in f64.

  python tools/bench_slim.py [--shape ml-100k|ml-20m] [--cols N] [--abs]

Workloads are synthetic (recommend-lib_amd/synthetic.py's degree model: lognormal user activity,
Zipf item popularity), the driver's defaults alpha 0.5, lam_bda 0.02, max_iter 1000, tol 1e-4:
  ml-100k  943 users x 1,682 items, ~100 k positives; every column
  ml-20m   138,493 users x 26,744 items, ~20 M positives; the first --cols columns (default 256)
One JSON line: Gram seconds and i8 op/s (2 U p^2, halved for symmetry), coordinate-descent
seconds, columns/s and moves/s, and the bytes/s of the moves' gradient updates (moves * p * 8:
one row of G read per move) beside the HBM rate of the MI355X guide.  --abs: absolute lambda.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"ml-100k": (943, 1682, 100_000), "ml-20m": (138_493, 26_744, 20_000_263)}
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak


def train_pairs(shape):
    syn = importlib.import_module("recommend-lib_amd.synthetic")
    U, p, npos = SHAPES[shape]
    return syn.make_positives(U, p, npos)


def run(shape, cols, absolute):
    rl = importlib.import_module("recommend-lib_amd")
    U, p, _ = SHAPES[shape]
    pairs = train_pairs(shape)
    m = rl.SLIM(pairs, num_user=U, num_item=p)
    m.gram(fetch=False)  # warm-up (kernel load)
    st_g = m.gram(fetch=False)
    n = p if cols is None else min(cols, p)
    m.fit(lambda_is_ratio=not absolute, columns=(0, min(n, 8)))  # warm-up
    m.fit(lambda_is_ratio=not absolute, columns=(0, n))
    st = m.last_stats
    ops = 2.0 * U * p * p / 2
    out = {"metric": "SLIM fit: Gram + coordinate descent (SLiMRecommender.py)",
           "value": round(st_g + st["cd_seconds"], 6), "unit": "s", "n_gpus": 1, "dtype": "i8 Gram, f64 descent",
           "data": f"synthetic {shape} shape ({U} users x {p} items, {len(pairs)} positives)",
           "config": {"alpha": 0.5, "lam_bda": 0.02, "max_iter": 1000, "tol": 1e-4,
                      "lambda_is_ratio": not absolute},
           "columns": n, "columns_bounded_by_cols": n < p,
           "gram_seconds": round(st_g, 6), "gram_i8_op_per_s": float(f"{ops / st_g:.4g}"),
           "cd_seconds": round(st["cd_seconds"], 6),
           "columns_per_s": round(st["columns"] / st["cd_seconds"], 1),
           "moves_per_s": round(st["moves"] / st["cd_seconds"], 1),
           "sweeps": st["sweeps"], "moves": st["moves"], "capped": st["capped"],
           "move_bytes_per_s": float(f"{st['moves'] * p * 8 / st['cd_seconds']:.4g}"),
           "hbm_bytes_per_s_guide": HBM_BYTES_PER_S,
           "nnz_W": int(np.count_nonzero(m.weights((0, n))))}
    m.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml-100k", choices=list(SHAPES))
    ap.add_argument("--cols", type=int, default=None)
    ap.add_argument("--abs", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (the HIP runtime the library binds to)
    run(a.shape, a.cols if a.cols is not None else (256 if a.shape == "ml-20m" else None), a.abs)


if __name__ == "__main__":
    main()
