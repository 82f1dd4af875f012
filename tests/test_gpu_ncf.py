"""GPU: the NCF path (include/ncf.h) against the reference's own recorded runs (G1,
tests/golden/ncf_steps_tiny.npz: NCF GMF / MLP / NeuMF-end, BCEWithLogitsLoss, Adam) and the
oracle (oracle/ncf_oracle.py).  Tolerances: forward 1e-6 (f32 MFMA vs torch f32); Adam steps
2e-5 absolute on O(0.01-0.3) weights (embedding gradients are f32 atomics: summation order
differs from torch's; Adam's first steps move every element by ~lr regardless of |g|)."""
import numpy as np
import pytest

from oracle import bpr_oracle as BO
from oracle import ncf_oracle as N

pytestmark = pytest.mark.gpu


def _cases(golden):
    f = golden("ncf_steps_tiny.npz")
    for c in range(int(f["n_cases"])):
        pre = f"c{c}_"
        d, L, B, steps, U, I = (int(x) for x in f[pre + "meta"])
        yield f, pre, str(f[pre + "model"]), d, L, B, steps, U, I


def _model(rl, f, pre, model, d, L, B, U, I):
    m = rl.NCF(U, I, d, L, model=model, batch_size=B, seed=1)
    m.load_state_dict({n: f[pre + "init_" + n] for n in m.names})
    return m


def test_forward_matches_reference(rl, golden):
    for f, pre, model, d, L, B, steps, U, I in _cases(golden):
        m = _model(rl, f, pre, model, d, L, B, U, I)
        z = m.predict_logits(f[pre + "u"][0], f[pre + "i"][0])
        np.testing.assert_allclose(z, f[pre + "pred0"], rtol=1e-5, atol=1e-6, err_msg=model)


def test_adam_steps_match_reference(rl, golden):
    for f, pre, model, d, L, B, steps, U, I in _cases(golden):
        m = _model(rl, f, pre, model, d, L, B, U, I)
        for k in range(steps):
            st = m.train_samples(f[pre + "u"][k], f[pre + "i"][k], f[pre + "y"][k])
            assert st["steps"] == 1
            assert abs(st["loss"] - f[pre + "loss"][k]) < 2e-6, (model, k)
            if k + 1 in (1, 3, steps):
                got = m.state_dict()
                for n in m.names:
                    np.testing.assert_allclose(got[n], f[pre + f"after{k + 1}_" + n], rtol=0,
                                               atol=2e-5, err_msg=f"{model} {n} step {k + 1}")


def test_larger_tower_matches_oracle(rl):
    """d=64, 3 layers (the C4 tower: 512 -> 256 -> 128 -> 64), B=256 with duplicates."""
    U, I, d, L, B = 300, 500, 64, 3, 256
    g = np.random.default_rng(5)
    m = rl.NCF(U, I, d, L, batch_size=B, seed=2)
    params = m.state_dict()
    opt = N.Adam(params)
    for k in range(4):
        u = g.integers(0, U, B)
        i = g.integers(0, I, B)
        u[:30] = 7
        y = (g.random(B) < 0.25).astype(np.float32)
        z = m.predict_logits(u, i)
        z_ref, _ = N.forward(params, "NeuMF-end", L, u, i)
        np.testing.assert_allclose(z, z_ref, rtol=1e-4, atol=2e-6)
        grads, loss = N.grads(params, "NeuMF-end", L, u, i, y)
        params = opt.step(params, grads)
        st = m.train_samples(u, i, y)
        assert abs(st["loss"] - loss) < 1e-5
    got = m.state_dict()
    for n in m.names:
        np.testing.assert_allclose(got[n], params[n], rtol=0, atol=5e-5, err_msg=n)


def test_lazy_embedding_adam_matches_dense_over_long_gaps(rl):
    """The embedding rows' zero-gradient Adam steps are applied lazily (k_ncf_catch_up, closed
    form) where torch's Adam moves every row with a nonzero moment every step: cold rows touched at
    steps 3 and 251 (248 zero-gradient steps between, more than the catch-up's 192 terms), a
    predict of cold rows at step 101 (catch-up of the rows read) and state_dict reads (every row)
    in between.  Against the oracle's dense Adam at 1e-6 (measured: 6e-8 lazy, 5e-8 for the dense
    sweep it replaced, tools/dbg/ncf_lazy_check.py)."""
    U, I, d, L, B = 40, 48, 8, 2, 8
    g = np.random.default_rng(17)
    m = rl.NCF(U, I, d, L, batch_size=B, seed=3)
    params = m.state_dict()
    opt = N.Adam(params)
    cold_u, cold_i = np.arange(3 * U // 4, U), np.arange(3 * I // 4, 3 * I // 4 + U // 4)
    seen_u, seen_i = set(), set()
    for k in range(260):
        u = g.integers(0, U // 4, B)
        i = g.integers(0, I // 4, B)
        if k in (2, 250):
            u[: B // 2] = g.integers(3 * U // 4, U, B // 2)
            i[: B // 2] = g.integers(3 * I // 4, I, B // 2)
        y = (g.random(B) < 0.3).astype(np.float32)
        seen_u.update(u.tolist())
        seen_i.update(i.tolist())
        grads, _ = N.grads(params, "NeuMF-end", L, u, i, y)
        params = opt.step(params, grads)
        m.train_samples(u, i, y)
        if k == 100:
            z = m.predict_logits(cold_u, cold_i)
            z_ref, _ = N.forward(params, "NeuMF-end", L, cold_u, cold_i)
            np.testing.assert_allclose(z, z_ref, rtol=0, atol=1e-6)
        if k + 1 in (50, 150, 251, 260):
            got = m.state_dict()
            for n in m.names:
                np.testing.assert_allclose(got[n], params[n], rtol=0, atol=1e-6, err_msg=f"{n} step {k + 1}")
    assert m.active_rows() == (len(seen_u), len(seen_i))
    m.close()


def test_lazy_adam_within_multi_step_calls_matches_dense(rl):
    """The same long-gap stream as above, replayed as two calls of many steps: inside a call the
    next step's rows are caught up beside the middle layers (k_ncf_mid's extra workgroups) and a
    step's row Adam runs in the next step's row launch (k_ncf_rows), both paths a one-step call
    never takes.  Against the oracle's dense Adam at 1e-6."""
    U, I, d, L, B = 40, 48, 8, 2, 8
    g = np.random.default_rng(29)
    m = rl.NCF(U, I, d, L, batch_size=B, seed=5)
    params = m.state_dict()
    opt = N.Adam(params)
    us, is_, ys = [], [], []
    for k in range(260):
        u = g.integers(0, U // 4, B)
        i = g.integers(0, I // 4, B)
        if k in (2, 250):
            u[: B // 2] = g.integers(3 * U // 4, U, B // 2)
            i[: B // 2] = g.integers(3 * I // 4, I, B // 2)
        u[B - 1], i[B - 1] = u[0], i[0]  # a repeated row inside the step
        y = (g.random(B) < 0.3).astype(np.float32)
        grads, _ = N.grads(params, "NeuMF-end", L, u, i, y)
        params = opt.step(params, grads)
        us.append(u), is_.append(i), ys.append(y)
    for lo, hi in ((0, 150), (150, 260)):
        st = m.train_samples(np.concatenate(us[lo:hi]), np.concatenate(is_[lo:hi]), np.concatenate(ys[lo:hi]))
        assert st["steps"] == hi - lo
    got = m.state_dict()
    for n in m.names:
        np.testing.assert_allclose(got[n], params[n], rtol=0, atol=1e-6, err_msg=n)
    m.close()


def test_sampler_matches_oracle_and_ncfdata_semantics(rl, golden):
    f = golden("bpr_ml100k_replay.npz")
    pos = f["positives"].astype(np.int64)
    U, I = int(f["U"]), int(f["I"])
    m = rl.NCF(U, I, 8, 1, batch_size=256, num_ng=4, seed=11)
    m.set_train(pos)
    n = m.epoch_size()[0]
    assert n == 5 * len(pos)
    u, i, y = m.sample(3, 0, n)
    indptr, indices = BO.build_csr(pos[:, 0], pos[:, 1], U)
    uo, io, yo = N.sample(pos[:, 0], pos[:, 1], indptr, indices, I, 4, 11, 3, 1000, 5000)
    assert np.array_equal(u[1000:6000], uo) and np.array_equal(i[1000:6000], io)
    assert np.array_equal(y[1000:6000], yo)
    # NCFData.ng_sample: every positive once (label 1) and 4 negatives per positive, none a positive
    assert int(y.sum()) == len(pos)
    posset = set(map(tuple, pos.tolist()))
    neg = y == 0
    assert not any((a, b) in posset for a, b in zip(u[neg].tolist(), i[neg].tolist()))
    cnt = np.bincount(u[neg], minlength=U)
    assert np.array_equal(cnt, 4 * np.bincount(pos[:, 0], minlength=U))


def test_training_reduces_loss_and_ranks(rl, golden):
    f = golden("bpr_ml100k_replay.npz")
    pos = f["positives"].astype(np.int64)
    U, I = int(f["U"]), int(f["I"])
    m = rl.NCF(U, I, 16, 2, batch_size=256, num_ng=4, seed=3, lr=0.001)
    m.set_train(pos)
    losses = [m.train_epoch()["loss"] / m.epoch_size()[1] for _ in range(3)]
    assert losses[-1] < losses[0] < 0.7, losses
    # positives now score above random items for most users
    g = np.random.default_rng(0)
    zp = m.predict_logits(pos[:2000, 0], pos[:2000, 1])
    zn = m.predict_logits(pos[:2000, 0], g.integers(0, I, 2000))
    assert (zp > zn).mean() > 0.75


# -- the handle's buffers and failure paths (csrc/ncf_capi.cpp): a tiny model, two train sets ----
TU, TI = 40, 48


def _tiny(rl, L=1, **kw):
    return rl.NCF(TU, TI, 8, L, batch_size=8, num_ng=2, seed=9, **kw)


def _train_sets():
    """A: 30 pairs; B: 200 pairs, the last 40 repeating the first 40."""
    g = np.random.default_rng(41)
    a = np.stack([g.integers(0, TU, 30), g.integers(0, TI, 30)], 1)
    b = np.stack([g.integers(0, TU, 200), g.integers(0, TI, 200)], 1)
    b[160:] = b[:40]
    return a, b


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def test_set_train_again_replaces_the_set(rl):
    sets = _train_sets()
    want = []
    for s in sets:  # a handle that only ever saw this set
        f = _tiny(rl).set_train(s)
        want.append((f.epoch_size(), f.sample(3)))
        f.close()
    assert want[0][0] == (90, 12) and want[1][0] == (600, 75)
    m = _tiny(rl)
    for k in (0, 1, 0):
        m.set_train(sets[k])
        assert m.epoch_size() == want[k][0]
        assert _same(m.sample(3), want[k][1])
    m.close()


def test_failed_set_train_keeps_the_previous_set(rl):
    a, _ = _train_sets()
    m = _tiny(rl).set_train(a)
    size, before = m.epoch_size(), m.sample(1)
    bad = a.copy()
    bad[17, 1] = TI
    with pytest.raises(ValueError, match="out of range"):
        m.set_train(bad)
    assert m.epoch_size() == size
    assert _same(m.sample(1), before)
    assert m.train_steps(0, 0, 2)["steps"] == 2
    m.close()


def test_empty_train_set_is_a_state_error(rl):
    a, _ = _train_sets()
    m = _tiny(rl).set_train(a)
    m.set_train(np.empty((0, 2), np.int64))
    assert m.epoch_size() == (0, 0)
    with pytest.raises(rl.BprmfError, match="error -4.*ncf_set_train first"):  # BPRMF_E_STATE
        m.train_steps(0, 0, 0)
    with pytest.raises(rl.BprmfError, match="error -4.*ncf_set_train first"):
        m.sample(0, 0, 0)
    m.close()


def test_rejected_configs_leave_a_usable_process(rl):
    """The last config passes the argument checks and is refused once the handle exists: the
    forward/backward workgroup's LDS plan (ncf.hip lds_plan) holds 4 * 16 + 2 * 16 (d + 4) +
    16 * sum_l (nout[l] + 4) floats, at 4 layers 448 + 272 d; d = 152 gives 41,792 floats =
    167,168 B > 160 KB = 163,840 B (d = 148: 162,816 B, accepted)."""
    with pytest.raises(rl.BprmfError, match="error -6"):  # BPRMF_E_UNSUPPORTED
        rl.NCF(TU, TI, 6, 1, batch_size=8)
    with pytest.raises(rl.BprmfError, match="error -6"):
        rl.NCF(TU, TI, 8, 5, batch_size=8)
    with pytest.raises(ValueError, match="batch_size"):
        rl.NCF(TU, TI, 8, 1, batch_size=8193)
    with pytest.raises(rl.BprmfError, match="error -6.*167168 B of LDS"):
        rl.NCF(4, 4, 152, 4, batch_size=8)
    m = _tiny(rl, L=2).set_train(_train_sets()[0])
    assert m.train_steps(0, 0, 2)["steps"] == 2
    m.close()


def test_long_predict_equals_its_slices(rl):
    """70,000 pairs: two chunks of the forward (65,536 + 4,464) and, as for every slice, the
    branch that brings every row to the current step first."""
    m = _tiny(rl, L=2).set_train(_train_sets()[1])
    m.train_steps(0, 0, 3)
    g = np.random.default_rng(43)
    n = 70_000
    u, i = g.integers(0, TU, n), g.integers(0, TI, n)
    z = m.predict_logits(u, i)
    parts = [m.predict_logits(u[s:s + 1000], i[s:s + 1000]) for s in range(0, n, 1000)]
    assert np.array_equal(z, np.concatenate(parts))
    assert np.isfinite(z).all() and np.unique(z).size > 100
    m.close()


def test_profile_counts_launches(rl):
    """One sampler launch per call; per step one row launch (the previous step's row Adam with
    this step's catch-up) and one forward/backward; the call's last row Adam runs alone."""
    m = _tiny(rl).set_train(_train_sets()[0])
    m.profile(True)
    m.train_steps(0, 0, 5)
    got = {k: v["count"] for k, v in m.profile_read().items()}
    assert got == dict(sample=1, fwd_bwd=5, adam=1, catch_up=5)
    m.profile(False)
    m.profile(True)
    m.train_steps(0, 5, 1)
    got = {k: v["count"] for k, v in m.profile_read().items()}
    assert got == dict(sample=1, fwd_bwd=1, adam=1, catch_up=1)
    m.close()
