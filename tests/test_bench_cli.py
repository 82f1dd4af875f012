"""bench.py's command line: --dump-outputs (what the timed steps computed, as .npy), --full (the
legs beside the headline) and the result line of a plain run."""
import json
import os

import numpy as np
import pytest

import bench

TINY = ["--gpus", "1", "--users", "700", "--items", "300", "--positives", "6000", "--factor", "32",
        "--batch-size", "256", "--steps", "3", "--warmup", "1"]


def test_dump_outputs_keeps_small_arrays_whole(tmp_path):
    P = np.arange(12, dtype=np.float32).reshape(4, 3)
    bench.dump_outputs(str(tmp_path / "d"), {"P": P, "loss": np.array([1.5])})
    got = np.load(tmp_path / "d" / "P.npy")
    assert got.dtype == np.float32 and np.array_equal(got, P)
    loss = np.load(tmp_path / "d" / "loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [1.5]


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    g = np.random.default_rng(3)
    P = g.standard_normal((300, 8)).astype(np.float32)   # 9600 B
    Q = g.standard_normal((100, 8)).astype(np.float32)   # 3200 B
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"P": P, "Q": Q}, suffix=".rank1")
    a = {n: np.load(tmp_path / "a" / f"{n}.rank1.npy") for n in ("P", "Q")}
    b = {n: np.load(tmp_path / "b" / f"{n}.rank1.npy") for n in ("P", "Q")}
    assert sum(v.nbytes for v in a.values()) <= 4096
    for n, full in (("P", P), ("Q", Q)):
        assert np.array_equal(a[n], b[n])
        assert 0 < len(a[n]) < len(full) and a[n].dtype == np.float32
        # rows of the table, in the table's order
        idx = [int(np.flatnonzero((full == r).all(axis=1))[0]) for r in a[n]]
        assert idx == sorted(set(idx))


def _run(argv, capsys, monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    out = bench.main()
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(line) == json.loads(json.dumps(out))
    return out


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_tables(rl, tmp_path, capsys, monkeypatch):
    outs = []
    for d in ("a", "b"):
        out = _run(TINY + ["--dump-outputs", str(tmp_path / d)], capsys, monkeypatch)
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
        assert out["value"] == pytest.approx(256 / (out["ms_per_step"] * 1e-3), rel=1e-3)
        assert out["unit"] == "triplets/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        # a plain run carries none of the legs that take runs of their own
        assert out["roofline"] is None and out["cpu_baseline"] is None
        assert "relaxed_local" not in out and "relaxed_local_hbm" not in out
        assert sorted(os.listdir(tmp_path / d)) == ["P.npy", "Q.npy", "loss.npy"]
        outs.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("P", "Q", "loss")})
    a, b = outs
    assert a["P"].shape == (700, 32) and a["Q"].shape == (300, 32) and a["P"].dtype == np.float32
    assert np.isfinite(a["loss"]).all() and a["loss"].dtype == np.float64
    # the tables after warm-up + timed steps: those of a model driven by hand over the same steps
    m = rl.BPRMF(700, 300, 32, lr=0.01, wd=0.001, batch_size=256, num_ng=4, seed=20261015, device=0)
    syn = __import__("importlib").import_module("recommend-lib_amd.synthetic")
    m.set_train(syn.make_positives(700, 300, 6000, 20261015))
    assert m.epoch_size()[1] >= 4
    m.train_steps(0, 0, 1)
    st = m.train_steps(0, 1, 3)
    P, Q = m.get_weights()
    for got in (a, b):  # same arguments, same inputs, the exact step: the same bits
        assert np.array_equal(got["P"], P) and np.array_equal(got["Q"], Q)
        assert got["loss"][0] == st["loss"]


@pytest.mark.gpu
def test_full_adds_the_event_pass(rl, capsys, monkeypatch):
    out = _run(TINY + ["--full", "--no-relaxed", "--no-cpu-baseline"], capsys, monkeypatch)
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["roofline"]["avg_us_per_step"] > 0 and out["cpu_baseline"] is None
