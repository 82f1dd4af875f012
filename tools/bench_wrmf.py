"""Measurement of WRMF (WRMFRecommender.py:37-56): implicit-feedback ALS epochs on the GPU in f64.

  python tools/bench_wrmf.py [--shape ml-100k|ml-20m|both] [--epochs E] [--heavy-nnz H]

Workloads are synthetic (recommend-lib_amd/synthetic.py's degree model: lognormal user activity,
Zipf item popularity), ratings 1..5, alpha 40, lambda 0.1:
  ml-100k  943 users x 1,682 items, ~100 k positives, d = 20 (the reference default)
  ml-20m   138,493 users x 26,744 items, ~20 M positives, d = 128
One JSON line per shape: seconds per epoch (device time), row solves per second, f64 FLOP/s from
the nominal count 2 (2 nnz d^2 + (U + I) d^3 / 3) + 2 (U + I) d^2 per epoch (both half-sweeps'
accumulation and Cholesky, and the two Gram matrices), the heavy rows per epoch, and at ml-100k
shape the host time of the numpy restatement (tests/wrmf_numpy.py) of the same epoch.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"ml-100k": (943, 1682, 100_000, 20), "ml-20m": (138_493, 26_744, 20_000_263, 128)}


def train_csr(U, I, npos, seed=7):
    syn = importlib.import_module("recommend-lib_amd.synthetic")
    pos = syn.make_positives(U, I, npos)  # ordered by user, items ascending within a user
    indptr = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(pos[:, 0], minlength=U), out=indptr[1:])
    r = np.random.default_rng(seed).integers(1, 6, len(pos)).astype(np.float64)
    return indptr, pos[:, 1].astype(np.int32), r, (U, I)


def run(shape, epochs, heavy_nnz, cpu):
    rl = importlib.import_module("recommend-lib_amd")
    U, I, npos, d = SHAPES[shape]
    csr = train_csr(U, I, npos)
    nnz = len(csr[1])
    m = rl.WRMF(csr, iterations=epochs, factor_num=d, heavy_nnz=heavy_nnz)
    X0, Y0 = m.factors()
    m.fit(1)  # warm-up (kernel load)
    m.set_factors(X0, Y0)
    t0 = time.perf_counter()
    m.fit(epochs)
    wall = time.perf_counter() - t0
    st = m.last_stats
    per_epoch = st["seconds"] / epochs
    flop = 2 * (2 * nnz * d * d + (U + I) * d ** 3 / 3) + 2 * (U + I) * d * d
    X, _ = m.factors()
    out = {"metric": "WRMF.fit ALS seconds per epoch (WRMFRecommender.py)", "value": round(per_epoch, 6),
           "unit": "s/epoch", "n_gpus": 1, "epochs": epochs, "dtype": "f64",
           "data": f"synthetic {shape} shape ({U} users x {I} items, {nnz} positives)",
           "config": {"factor_num": d, "alpha": 40, "lambda_val": 0.1, "gram": "reference",
                      "heavy_nnz": heavy_nnz or "default"},
           "solves_per_s": round(st["solves"] / st["seconds"], 1),
           "f64_flop_per_s": float(f"{flop / per_epoch:.4g}"), "flop_per_epoch": float(f"{flop:.4g}"),
           "heavy_rows": st["heavy_rows"] // epochs, "device_seconds": round(st["seconds"], 4),
           "wall_seconds_fit": round(wall, 4), "finite": bool(np.isfinite(X).all())}
    m.close()
    if cpu:
        import wrmf_numpy as W
        conf = (csr[0], csr[1], 40 * csr[2], csr[3])
        t0 = time.perf_counter()
        W.fit(conf, X0, Y0, 0.1, 1)
        out["cpu_baseline"] = {"value": round(time.perf_counter() - t0, 4), "unit": "s/epoch",
                               "kind": "numpy restatement (tests/wrmf_numpy.py), one epoch on the host"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["ml-100k", "ml-20m", "both"])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--heavy-nnz", type=int, default=0)
    a = ap.parse_args()
    import torch  # noqa: F401  (the HIP runtime the library binds to)
    for shape in (("ml-100k", "ml-20m") if a.shape == "both" else (a.shape,)):
        run(shape, a.epochs, a.heavy_nnz, cpu=shape == "ml-100k")


if __name__ == "__main__":
    main()
