"""ComplEx on the GPU (k_step_complex, k_score_complex, k_score_queries_complex: complex.hip; both optimizer passes)
against the float64 reference tests/complex_reference.py and the reference implementation's own runs
(tests/golden/complex_*.npz).

Gradient parity runs SGD at lr 1 on explicit batches (complex_cases.py), so the table delta is the gradient:
    |delta_gpu - delta_ref64| <= tol = min(1e-5, max(4 * 2^-23 * max(1, |g|max), 4 * GRAD_DEV[family]))
for every cell of the four tables, and the loss within min(1e-5, 4 LOSS_DEV) of max(1, |loss|). Scores:
    |got - ref64| <= tol(D) * max(1, |ref64|),  tol(D) = min(1e-5, max(4 * 2^-23, 4 * SCORE_DEV[D])).
The input conditions of the seeds are asserted on the CPU in test_complex_reference_cpu.py (among them: a kernel with
the sign of the h_im t_re r_im term wrong, or one that ignores the im tables, moves cells of all four tables by more
than 20 bounds). Every test prints its observed maxima.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import complex_cases as cc
import complex_reference as cr
import oracle
from conftest import KG_SMALL
from helpers import golden, load

pytestmark = pytest.mark.gpu

B1, B2 = 0.9, 0.999
PT_EINVAL, PT_ENOTSUP = 1, 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible HIP device"


def _model(tabs, dim):
    from openke.module.model import ComplEx
    kge = ComplEx(tabs[0].shape[0], tabs[2].shape[0], dim=dim)
    _set_tables(kge, tabs)
    return kge


def _set_tables(kge, tabs):
    for name, x in zip(cr.TABLES, tabs):
        getattr(kge, name).weight.data.copy_(torch.from_numpy(np.asarray(x)))


def _loss(cfg):
    from openke.module.loss import SigmoidLoss, SoftplusLoss
    cls = SigmoidLoss if cfg["loss"] == "sigmoid" else SoftplusLoss
    return cls(adv_temperature=cfg["adv_temperature"])


def _trainer(tabs, cfg, opt, lr):
    """(kge, Trainer) for a ComplEx holding the given tables, on the GPU."""
    from openke.config import Trainer
    from openke.module.strategy import NegativeSampling
    kge = _model(tabs, cfg["dim"])
    ns = NegativeSampling(model=kge, loss=_loss(cfg), batch_size=cfg["batch_size"], regul_rate=cfg["regul_rate"])
    ns.cuda()
    return kge, Trainer(model=ns, data_loader=None, train_times=0, alpha=lr, use_gpu=True, opt_method=opt)


def _tables(kge):
    """The four tables in complex_reference.TABLES' order."""
    return [getattr(kge, name).weight.detach().cpu().numpy().copy() for name in cr.TABLES]


def _by_name(kge, per_model_table):
    """A per-table tuple in the model's tables() order (ent_re, rel_re, -, ent_im, rel_im), in TABLES' order."""
    return [per_model_table[i] for i in (0, 3, 1, 4)]


def _check_step(tag, tabs, got, grads, aux, cfg, loss, want_loss, transform=None):
    tol = cr.grad_bound(cr.family(cfg), aux["gmax"])
    devs = []
    for i in range(4):
        want = grads[i] if transform is None else transform(i, grads[i])
        dev = float(np.abs((np.asarray(tabs[i], dtype=np.float64) - got[i].astype(np.float64)) - want).max())
        print("%s %s: max |delta_gpu - delta_ref64| %.3e (tol %.3e, |g|max %.3e)" % (tag, cr.TABLES[i], dev, tol,
                                                                                   aux["gmax"]))
        devs.append(dev)
    print("%s loss gpu %.9g ref %.9g (rel %.3e, tol %.3e)" % (tag, loss, want_loss, abs(loss - want_loss) /
                                                             max(1.0, abs(want_loss)), cr.loss_tol()))
    for i, dev in enumerate(devs):
        assert dev <= tol, (tag, cr.TABLES[i], dev, tol)
    assert cr.loss_close(loss, want_loss), (loss, want_loss)


def _free_rows_identical(got, tabs):
    for i in range(4):
        row = cc.FREE_ENT if i < 2 else cc.FREE_REL
        np.testing.assert_array_equal(got[i][row], tabs[i][row])


# ------------------------------------------------------------------ 1. gradient parity ----------
@pytest.mark.parametrize("case", cc.GRAD_CASES + [cc.THRESHOLD_CASE, cc.MANY_REL_CASE], ids=lambda c: c[0])
def test_gradient_parity_sgd(case):
    tabs, hrt, cfg = cc.build(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = cr.loss_and_grads(tabs, *hrt, bs, cfg)
    kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
    loss = trn.train_one_step(cc.as_batch(hrt))
    got = _tables(kge)
    _check_step(case[0], tabs, got, grads, aux, cfg, loss, want_loss)
    # the entity and the relation no slot names: their four rows bit-identical
    _free_rows_identical(got, tabs)
    # gradient rows and flags are back to zero: the same step from the same tables gives the same tables and loss
    # to the bound again (a leftover gradient row would double a delta)
    _set_tables(kge, tabs)
    loss2 = trn.train_one_step(cc.as_batch(hrt))
    _check_step(case[0] + " again", tabs, _tables(kge), grads, aux, cfg, loss2, want_loss)


# ------------------------------------------------------------------ 2. Adagrad, Adam -------------
def test_gradient_parity_adagrad_with_regul_rate():
    """The same step through Adagrad (k_apply, twice) from a given state_sum in [1, 2): |d delta / d g| <= 1 there, so
    the gradient bound holds for the delta; the four tables and their state against torch's Adagrad formula on the
    float64 gradients."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, hrt, cfg = cc.build(cc.ADAGRAD_CASE)
    bs = cfg["batch_size"]
    want_loss, grads, aux = cr.loss_and_grads(tabs, *hrt, bs, cfg)
    kge, trn = _trainer(tabs, cfg, "adagrad", 1.0)
    trn.optimizer = NativeOptimizer(_native.PT_ADAGRAD, 1.0, kge.tables())
    rng = np.random.default_rng(77)
    state = [rng.uniform(1, 2, size=t.shape).astype(np.float32) for t in tabs]
    assert [s is None for s in trn.optimizer.state_sum] == [False, False, True, False, False]
    sums = _by_name(kge, trn.optimizer.state_sum)
    for s, x in zip(sums, state):
        s.copy_(torch.from_numpy(x))
    loss = trn.train_one_step(cc.as_batch(hrt))
    got = _tables(kge)
    _check_step("adagrad", tabs, got, grads, aux, cfg, loss, want_loss,
                lambda i, g: g / (np.sqrt(state[i].astype(np.float64) + g ** 2) + 1e-10))
    # torch.optim.Adagrad itself on the float64 gradients gives the same tables
    ws = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in tabs]
    topt = torch.optim.Adagrad(ws, lr=1.0)
    for w, s, g in zip(ws, state, grads):
        topt.state[w]["sum"] = torch.tensor(s, dtype=torch.float64)
        w.grad = torch.tensor(g)
    topt.step()
    tol = cr.grad_bound(cr.family(cfg), aux["gmax"])
    for i, w in enumerate(ws):
        assert float(np.abs(got[i] - w.detach().numpy()).max()) <= tol
    for i, s in enumerate(sums):
        dev = float(np.abs(s.cpu().numpy().astype(np.float64) - (state[i].astype(np.float64) + grads[i] ** 2)).max())
        assert dev <= 2.0 ** -22 + 2 * aux["gmax"] * tol, (i, dev)
    _free_rows_identical(got, tabs)


@pytest.mark.parametrize("case", cc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_three_steps_from_given_state(case):
    """After every step, for the four tables: exp_avg / exp_avg_sq within (1 - b1) tol / (1 - b2) 2 |g|max tol of the
    float64 update at the GPU's own pre-step state, every weight the float64 update formula at the GPU's own new
    moments (4 ulp of w + 1e-6 |delta|), the loss. Entity 36 and relation 2 never occur in a batch and start with zero
    moments: their four rows and moments stay bit-identical."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, batches, cfg, (m0, v0), lr, step0 = cc.build_adam(case)
    bs = cfg["batch_size"]
    kge, trn = _trainer(tabs, cfg, "adam", lr)
    trn.optimizer = NativeOptimizer(_native.PT_ADAM, lr, kge.tables())
    opt = trn.optimizer
    ms, vs = _by_name(kge, opt.exp_avg), _by_name(kge, opt.exp_avg_sq)
    for dst, src in zip(ms + vs, m0 + v0):
        dst.copy_(torch.from_numpy(src))
    opt.step = step0

    def state():
        return [x.detach().cpu().numpy().copy() for x in ms], [x.detach().cpu().numpy().copy() for x in vs]

    w = _tables(kge)
    m, v = state()
    for s, hrt in enumerate(batches):
        want_loss, grads, aux = cr.loss_and_grads(w, *hrt, bs, cfg)
        loss = trn.train_one_step(cc.as_batch(hrt))
        assert opt.step == step0 + s + 1
        print("%s step %d loss gpu %.9g ref %.9g" % (case[0], s, loss, want_loss))
        assert cr.loss_close(loss, want_loss), (loss, want_loss)
        w2 = _tables(kge)
        m2, v2 = state()
        tol = cr.grad_bound(cr.family(cfg), aux["gmax"])
        for i in range(4):
            _, mr, vr = cr.adam_update(w[i], m[i], v[i], grads[i], lr, opt.step)
            dm, dv = float(np.abs(m2[i] - mr).max()), float(np.abs(v2[i] - vr).max())
            print("%s step %d %s: |m - ref| %.3e (bound %.3e), |v - ref| %.3e (bound %.3e)"
                  % (case[0], s, cr.TABLES[i], dm, (1 - B1) * tol, dv, (1 - B2) * 2 * aux["gmax"] * tol))
            assert dm <= (1 - B1) * tol
            assert dv <= (1 - B2) * 2 * aux["gmax"] * tol
            wr = cr.adam_weights(w[i], m2[i], v2[i], lr, opt.step)
            bound = 4 * np.spacing(np.abs(w[i])).astype(np.float64) + 1e-6 * np.abs(wr - w[i])
            assert (np.abs(w2[i].astype(np.float64) - wr) <= bound).all(), (case[0], s, i)
            row = cc.FREE_ENT if i < 2 else cc.FREE_REL
            assert (w2[i][row] == tabs[i][row]).all() and not m2[i][row].any() and not v2[i][row].any()
        w, m, v = w2, m2, v2


# ------------------------------------------------------------------ 3. reference runs ------------
@pytest.mark.parametrize("path", golden("complex_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_reference_steps_teacher_forced(path):
    """Every recorded step of the reference implementation, from its own tables before the step: the GPU delta within
    the parity bound of the float64 gradient, the loss within the loss bound of float64 and twice that of the recorded
    float32 one."""
    z = load(path)
    cfg = cr.golden_cfg(z)
    bs = cfg["batch_size"]
    for s in range(int(z["steps"])):
        tabs = [np.array(x) for x in cr.golden_tables(z, "s%d" % s)]
        h, t, r = cr.golden_step(z, s)
        want_loss, grads, aux = cr.loss_and_grads(tabs, h, t, r, bs, cfg)
        kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
        loss = trn.train_one_step({"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"})
        _check_step("%s step %d" % (path.split("/")[-1], s), tabs, _tables(kge), grads, aux, cfg, loss, want_loss)
        rec = float(z["losses"][s])
        assert abs(loss - rec) <= 2 * cr.loss_tol() * max(1.0, abs(rec)), (loss, rec)


@pytest.mark.parametrize("path", golden("complex_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_optimizer_runs_match_reference_trajectories(path):
    """The reference implementation's 10-step Adagrad (regul_rate 1, bern: the example in miniature) and Adam runs:
    losses to rtol 1e-4, the optimizer state after step 1 (Adagrad sums / Adam moments), every table element within the
    caps of test_gpu_distmult.py's test of the same name. A sanity cap: the parity proof is the tests above."""
    z = load(path)
    cfg = cr.golden_cfg(z)
    lr, steps, opt = float(z["lr"]), int(z["steps"]), str(z["optimizer"])
    kge, trn = _trainer([np.array(x) for x in cr.golden_tables(z, "init")], cfg, opt, lr)
    for s in range(steps):
        h, t, r = cr.golden_step(z, s)
        loss = trn.train_one_step({"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"})
        assert abs(loss - float(z["losses"][s])) <= 1e-4 * abs(float(z["losses"][s])), (s, loss, float(z["losses"][s]))
        if s == 0:
            o = trn.optimizer
            for k, name in enumerate(cr.TABLES):
                if opt == "adam":
                    np.testing.assert_allclose(_by_name(kge, o.exp_avg)[k].cpu().numpy(), z["step1_m_" + name],
                                               rtol=0, atol=1e-7)
                    np.testing.assert_allclose(_by_name(kge, o.exp_avg_sq)[k].cpu().numpy(), z["step1_v_" + name],
                                               rtol=0, atol=1e-9)
                else:
                    np.testing.assert_allclose(_by_name(kge, o.state_sum)[k].cpu().numpy(), z["step1_sum_" + name],
                                               rtol=0, atol=1e-9)
    if opt == "adam":
        assert trn.optimizer.step == steps
    cap = 2 * steps * lr * (1 - B1) / np.sqrt(1 - B2) if opt == "adam" else steps * lr * 1e-3
    for got, want, name in zip(_tables(kge), cr.golden_tables(z, "final"), cr.TABLES):
        dev = float(np.abs(got - want).max())
        print("%s %s: |final - ref| %.3e (cap %.3e)" % (path.split("/")[-1], name, dev, cap))
        assert dev <= cap


# ------------------------------------------------------------------ 4. scores --------------------
def _rows(kge, fn, side, qh, qt, qr):
    from openke import _native
    dev = kge.ent_embeddings.weight.device
    E = kge.ent_embeddings.weight.shape[0]
    q = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(dev) for x in (qh, qt, qr)]
    out = torch.full((len(qh), E), -1.0, dtype=torch.float32, device=dev)
    desc = kge.native_desc()
    _native.check(fn(ctypes.byref(desc), side, _native.ptr(q[0]), _native.ptr(q[1]), _native.ptr(q[2]), len(qh),
                     _native.ptr(out), _native.stream()))
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("path", golden("complex_p*.npz"), ids=lambda p: p.split("/")[-1])
def test_predict_matches_reference(path):
    """predict (-s) in the three modes against the reference implementation's own float32 values; forward is its
    negative."""
    z = load(path)
    D = int(z["dim"])
    kge = _model(cr.golden_tables(z, ""), D).cuda()
    tol = cr.score_tol(D)
    for mode in ("normal", "head_batch", "tail_batch"):
        data = {"batch_h": z[mode + "_h"], "batch_t": z[mode + "_t"], "batch_r": z[mode + "_r"], "mode": mode}
        got = kge.predict(data).astype(np.float64)
        want = z[mode + "_score"].astype(np.float64)
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print("%s %s: worst %.3e (tol %.3e)" % (path.split("/")[-1], mode, float(err.max()), tol))
        assert (err <= tol).all(), (mode, float(err.max()), tol)
        fwd = kge.forward(data).cpu().numpy()
        np.testing.assert_array_equal(-fwd, kge.predict(data))


# queries per lane group of k_score_queries_complex (complex.hip: 4 where a lane holds up to 8 floats of a row, else 2)
QT_MAX = 4


@pytest.mark.parametrize("D", cr.SCORE_DIMS)
def test_scores_match_float64(D):
    """pt_score in the three modes (through predict), pt_score_queries and pt_score_rows on both sides, cell by cell;
    nq = 1, QT + 1 and a count that is no multiple of QT (for QT = 2 and 4 alike); the truth entity first, last and in
    the middle of the candidate order."""
    from openke import _native
    L = _native.lib()
    tol = cr.score_tol(D)
    worst = 0.0
    tabs, batches = cr.score_case(D)
    kge = _model(tabs, D).cuda()
    for mode, (h, t, r) in batches.items():
        got = kge.predict({"batch_h": h, "batch_t": t, "batch_r": r, "mode": mode}).astype(np.float64)
        ref = -cr.scores(tabs, *cr.expand_predict(h, t, r, mode))
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert (err <= tol).all(), (D, mode, float(err.max()), tol)
    h, t, r = (x.copy() for x in batches["normal"])
    # truth first (entity 0), last (E - 1) and in the middle, on either side
    h[0], t[0], h[1], t[1], h[2], t[2] = 0, 0, cr.E - 1, cr.E - 1, cr.E // 2, cr.E // 2
    for nq in (1, QT_MAX + 1, 7):
        for side in (0, 1):
            ref = np.stack([cr.lp_scores(tabs, int(t[i] if side == 0 else h[i]), int(r[i]), side) for i in range(nq)])
            rows = _rows(kge, L.pt_score_rows, side, h[:nq], t[:nq], r[:nq])
            err = np.abs(rows - ref) / np.maximum(1.0, np.abs(ref))
            worst = max(worst, float(err.max()))
            assert (err <= tol).all(), (D, side, "rows", float(err.max()), tol)
            cand = _rows(kge, L.pt_score_queries, side, h[:nq], t[:nq], r[:nq])
            for i in range(nq):   # candidate order [truth, 0..E-1 without truth]
                truth = int(h[i] if side == 0 else t[i])
                order = oracle.candidates(cr.E, truth)
                np.testing.assert_array_equal(cand[i], rows[i][order])
    print("D %d: worst |gpu - ref64| / max(1, |ref64|) %.3e (tol %.3e)" % (D, worst, tol))


# ------------------------------------------------------------------ 5. link prediction ----------
def test_link_prediction_matches_reference_ranks():
    """Tester.run_link_prediction on kg_small with the recorded tables: the metrics and every query's raw and filtered
    rank equal to the reference's, exactly (test_complex_reference_cpu.py asserts that the fixture has no near-tie)."""
    from openke.config import Tester
    from openke.data import TestDataLoader
    z = load(golden("complex_lp.npz")[0])
    tabs = cr.golden_tables(z, "")
    test_dl = TestDataLoader(KG_SMALL, "link")
    kge = _model(tabs, int(z["dim"]))
    tester = Tester(model=kge, data_loader=test_dl, use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    qs = z["queries"].astype(np.int64)
    h, t, r = test_dl.eval_triples()
    np.testing.assert_array_equal(np.stack([h, t, r], 1), qs)
    want = z["ranks"].astype(np.int64)
    for k, g in enumerate(tester.last_ranks):
        np.testing.assert_array_equal(np.asarray(g, dtype=np.int64), want[k], err_msg=str(z["rank_names"][k]))
    np.testing.assert_array_equal(np.array(res, dtype=np.float32), z["metrics"].astype(np.float32))


# ------------------------------------------------------------------ 6. checkpoints, Trainer.run --
def test_checkpoint_round_trip_and_reference_state_dict(tmp_path):
    """save_checkpoint -> a fresh ComplEx -> load_checkpoint gives the same scores; a state_dict with the reference's
    keys, built from fixture tables and written by torch.save, loads through load_checkpoint and scores as the fixture."""
    from openke.module.model import ComplEx
    z = load(golden("complex_p2.npz")[0])
    D = int(z["dim"])
    tabs = cr.golden_tables(z, "")
    kge = _model(tabs, D).cuda()
    data = {"batch_h": z["normal_h"], "batch_t": z["normal_t"], "batch_r": z["normal_r"], "mode": "normal"}
    before = kge.predict(data)
    path = os.path.join(str(tmp_path), "complex.ckpt")
    kge.save_checkpoint(path)
    torch.manual_seed(99)
    fresh = ComplEx(ent_tot=tabs[0].shape[0], rel_tot=tabs[2].shape[0], dim=D).cuda()
    assert not np.array_equal(fresh.predict(data), before)
    fresh.load_checkpoint(path)
    np.testing.assert_array_equal(fresh.predict(data), before)
    assert sorted(torch.load(path).keys()) == [str(k) for k in z["state_keys"]]
    sd = {k + ".weight": torch.from_numpy(np.array(x)) for k, x in zip(cr.TABLES, tabs)}
    sd.update({"zero_const": torch.Tensor([0]), "pi_const": torch.Tensor([3.14159265358979323846])})
    path2 = os.path.join(str(tmp_path), "reference.ckpt")
    torch.save(sd, path2)
    torch.manual_seed(100)
    other = ComplEx(ent_tot=tabs[0].shape[0], rel_tot=tabs[2].shape[0], dim=D).cuda()
    other.load_checkpoint(path2)
    np.testing.assert_array_equal(other.predict(data), before)


def test_trainer_run_with_the_examples_settings():
    """Trainer.run() in the shape of examples/train_complex_WN18.py on kg_small (normal sampling with bern, SoftplusLoss,
    regul_rate 1, Adagrad lr 0.5, dim 20) for three epochs: the losses are finite and decrease, and equal those of the
    same batches fed step by step to a second model; then Tester.run_link_prediction."""
    from openke.config import Tester, Trainer
    from openke.data import TestDataLoader, TrainDataLoader
    from openke.module.loss import SoftplusLoss
    from openke.module.model import ComplEx
    from openke.module.strategy import NegativeSampling
    bs, neg, seed, epochs = 150, 8, 33, 3

    def setup():
        dl = TrainDataLoader(in_path=KG_SMALL, batch_size=bs, threads=8, sampling_mode="normal", bern_flag=1,
                             filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
        torch.manual_seed(6)
        kge = ComplEx(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=20)
        ns = NegativeSampling(model=kge, loss=SoftplusLoss(), batch_size=dl.get_batch_size(), regul_rate=1.0)
        return dl, kge, Trainer(model=ns, data_loader=dl, train_times=epochs, alpha=0.5, use_gpu=True,
                                opt_method="adagrad")

    dl, kge, trn = setup()
    trn.run()
    assert not trn.last_run_fused
    assert len(trn.epoch_losses) == epochs and np.isfinite(trn.epoch_losses).all()
    assert trn.epoch_losses[-1] < trn.epoch_losses[0]
    # the same batches (the loader's own sampling call draws the stream the GPU sampler drew) step by step
    dl2, kge2, trn2 = setup()
    sums = []
    for _ in range(epochs):
        sums.append(sum(trn2.train_one_step(dl2.sampling()) for _ in range(dl2.nbatches)))
    print("epoch losses run %s, step by step %s" % (trn.epoch_losses, sums))
    np.testing.assert_allclose(trn.epoch_losses, sums, rtol=1e-4)
    for a, b in zip(_tables(kge), _tables(kge2)):
        assert float(np.abs(a - b).max()) <= 1e-4
    tester = Tester(model=kge, data_loader=TestDataLoader(KG_SMALL, "link"), use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    assert np.isfinite(np.asarray(res, dtype=np.float64)).all()


# ------------------------------------------------------------------ 7. refusals -----------------
def test_unsupported_python_combinations_raise():
    """MarginLoss, l3_regul_rate, deterministic=True, a head_batch batch, a cross-sampling loader and a universe
    configuration with ComplEx: NotImplementedError by name, the tables untouched."""
    from openke.config import Parallel_Universe_Config, Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss, SigmoidLoss, SoftplusLoss
    from openke.module.model import ComplEx
    from openke.module.strategy import NegativeSampling
    normal = {"batch_h": np.array([0, 1, 2, 3]), "batch_t": np.array([1, 2, 3, 4]), "batch_r": np.array([0, 1, 0, 1]),
              "mode": "normal"}
    head = {"batch_h": np.array([0, 1, 2, 3]), "batch_t": np.array([1, 2]), "batch_r": np.array([0, 1]),
            "mode": "head_batch"}
    cross = TrainDataLoader(in_path=KG_SMALL, batch_size=50, threads=8, sampling_mode="cross", bern_flag=0,
                            filter_flag=1, neg_ent=2, random_seed=3)
    cases = [
        (SigmoidLoss(adv_temperature=2), {}, {"deterministic": True}, normal, "not implemented for ComplEx"),
        (MarginLoss(margin=1.0), {}, {}, normal, "MarginLoss on ComplEx"),
        (SoftplusLoss(), {"l3_regul_rate": 0.1}, {"opt_method": "adam"}, normal, "l3_regul_rate on ComplEx"),
        (SoftplusLoss(), {}, {}, head, "ComplEx trains normal-mode batches only"),
        (SoftplusLoss(), {}, {"data_loader": cross}, normal, "ComplEx trains on normal sampling only"),
    ]
    for loss, ns_kw, tr_kw, batch, frag in cases:
        torch.manual_seed(1)
        kge = ComplEx(6, 2, dim=8)
        ns = NegativeSampling(model=kge, loss=loss, batch_size=2, **ns_kw)
        w0 = [t.detach().clone() for t in kge.tables() if t is not None]
        kw = dict({"data_loader": None}, **tr_kw)
        trn = Trainer(model=ns, train_times=1, alpha=0.1, use_gpu=True, **kw)
        with pytest.raises(NotImplementedError, match=frag):
            trn.train_one_step(batch)
        if kw["data_loader"] is not None:
            with pytest.raises(NotImplementedError, match=frag):
                trn.run()
        for a, b in zip(w0, [t for t in kge.tables() if t is not None]):
            assert torch.equal(a, b.detach().cpu())
    pu = object.__new__(Parallel_Universe_Config)
    pu.embedding_model = ComplEx
    with pytest.raises(NotImplementedError, match="ComplEx"):
        pu._check_setup()
    # tables of unequal shapes are refused before any native call
    kge = ComplEx(6, 2, dim=8).cuda()
    kge.ent_im_embeddings = torch.nn.Embedding(5, 8).cuda()
    with pytest.raises(RuntimeError, match="ComplEx"):
        kge.native_desc()


def test_unsupported_native_combinations_are_refused():
    """Every PT_COMPLEX refusal of the C ABI: PT_ENOTSUP / PT_EINVAL with a message that names the model, rows,
    moments and the Adam step count untouched."""
    from openke import _native
    from openke.data import TrainDataLoader
    L = _native.lib()
    dev = torch.device("cuda", 0)
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=50, threads=8, bern_flag=0, filter_flag=1, neg_ent=2,
                         random_seed=3)
    sampler = dl.device_sampler()
    E, R, D = dl.get_ent_tot(), dl.get_rel_tot(), 8
    tabs = [torch.rand(E, D, device=dev) - 0.5, torch.rand(R, D, device=dev) - 0.5,
            torch.rand(E, D, device=dev) - 0.5, torch.rand(R, D, device=dev) - 0.5]   # ent_re, rel_re, ent_im, rel_im
    keep = [x.clone() for x in tabs]
    moments = [torch.zeros_like(x) for x in tabs + tabs]
    losses = torch.zeros(4, device=dev)
    st = _native.stream()
    PT = _native.PT_COMPLEX

    def desc(opt, im=True):
        d = _native.ModelDesc()
        d.model, d.p_norm, d.norm_flag, d.opt, d.lr, d.margin = PT, 7, 0, opt, 0.1, 2.0   # (p_norm is not read)
        d.ent_total, d.rel_total, d.dim = E, R, D
        d.ent, d.rel = tabs[0].data_ptr(), tabs[1].data_ptr()
        if im:
            d.ent_transfer, d.rel_transfer = tabs[2].data_ptr(), tabs[3].data_ptr()
        return d

    def trainer(opt):
        h = ctypes.c_void_p()
        d = desc(opt)
        _native.check(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)))
        return h

    def expect(rc_, code, *words):
        assert rc_ == code, (rc_, L.pt_last_error().decode())
        msg = L.pt_last_error().decode()
        assert all(w in msg for w in words), msg

    def loss_desc(kind, adv, flag):
        ld = _native.LossDesc()
        ld.kind, ld.adv, ld.temperature, ld.score_margin_flag, ld.score_margin = kind, adv, 1.0, flag, 6.0
        return ld

    def regul(rate, l3, mode):
        rd = _native.RegulDesc()
        rd.regul_rate, rd.l3_regul_rate, rd.batch_mode = rate, l3, mode
        return rd

    assert L.pt_version() == 1
    h = ctypes.c_void_p()
    # null im tables; Adagrad without the im tables' sums
    d = desc(_native.PT_SGD, im=False)
    expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), PT_EINVAL, "PT_COMPLEX", "im tables")
    out = torch.full((4,), 7.0, device=dev)
    idx = torch.zeros(4, dtype=torch.int64, device=dev)
    expect(L.pt_score(ctypes.byref(d), 0, _native.ptr(idx), _native.ptr(idx), _native.ptr(idx), 4, _native.ptr(out),
                      st), PT_EINVAL, "PT_COMPLEX")
    d = desc(_native.PT_ADAGRAD)
    d.ent_acc, d.rel_acc = moments[0].data_ptr(), moments[1].data_ptr()
    expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), PT_EINVAL, "Adagrad")
    # the dim rule is TransE's; the query answers 0 for the id
    for dim, ok in ((1, True), (511, True), (513, False), (516, True), (1024, True), (1028, False)):
        assert L.pt_model_dim_supported(dim, PT) == 0
        wide = [torch.zeros(4, dim, device=dev), torch.zeros(2, dim, device=dev)]
        d = desc(_native.PT_SGD)
        d.ent_total, d.rel_total, d.dim = 4, 2, dim
        d.ent, d.rel, d.ent_transfer, d.rel_transfer = (wide[0].data_ptr(), wide[1].data_ptr(), wide[0].data_ptr(),
                                                        wide[1].data_ptr())
        if ok:
            _native.check(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)))
            L.pt_trainer_free(h)
        else:
            expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), PT_ENOTSUP, "ComplEx", str(dim))
    b = [torch.zeros(50 * 3, dtype=torch.int64, device=dev) for _ in range(3)]

    def step(t, bs=50, neg=2, arrays=b):
        return L.pt_trainer_step(t, None, bs, neg, 0, 0, _native.ptr(arrays[0]), _native.ptr(arrays[1]),
                                 _native.ptr(arrays[2]), _native.ptr(losses), st)

    # SGD trainer: no captured run, no in-kernel sampling, no timed run, no reference-order mode
    t = trainer(_native.PT_SGD)
    ms4 = (ctypes.c_float * 4)()
    expect(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), PT_ENOTSUP, "PT_COMPLEX",
           "external batches")
    expect(L.pt_trainer_step(t, sampler, 50, 2, 0, 1, None, None, None, _native.ptr(losses), st), PT_ENOTSUP,
           "PT_COMPLEX")
    expect(L.pt_trainer_run_timed(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), ms4, st), PT_ENOTSUP, "PT_COMPLEX")
    expect(L.pt_trainer_set_deterministic(t, 1), PT_ENOTSUP, "PT_COMPLEX")
    # no loss set (the default is the margin loss), PT_LOSS_MARGIN, a model margin
    expect(step(t), PT_ENOTSUP, "PT_COMPLEX", "PT_LOSS_MARGIN")
    ld = loss_desc(_native.PT_LOSS_MARGIN, 1, 0)
    expect(L.pt_trainer_set_loss(t, ctypes.byref(ld)), PT_ENOTSUP, "PT_COMPLEX", "PT_LOSS_MARGIN")
    ld = loss_desc(_native.PT_LOSS_SIGMOID, 1, 1)
    expect(L.pt_trainer_set_loss(t, ctypes.byref(ld)), PT_ENOTSUP, "PT_COMPLEX", "model margin")
    ld = loss_desc(_native.PT_LOSS_SIGMOID, 1, 0)
    _native.check(L.pt_trainer_set_loss(t, ctypes.byref(ld)))
    # the regulariser descriptor: batch_mode 0 only, no l3
    for rd in (regul(-1.0, 0.0, 0), regul(float("nan"), 0.0, 0)):
        expect(L.pt_trainer_set_regul(t, ctypes.byref(rd)), PT_EINVAL, "regul_rate")
    for mode in (1, 2):
        rd = regul(1.0, 0.0, mode)
        expect(L.pt_trainer_set_regul(t, ctypes.byref(rd)), PT_ENOTSUP, "PT_COMPLEX", "batch_mode")
    rd = regul(0.0, 1e-3, 0)
    expect(L.pt_trainer_set_regul(t, ctypes.byref(rd)), PT_ENOTSUP, "PT_COMPLEX", "l3")
    rd = regul(1.0, 0.0, 0)
    _native.check(L.pt_trainer_set_regul(t, ctypes.byref(rd)))
    # neg past the LDS score buffer
    big = 16384
    hb = [torch.zeros(2 * (big + 1), dtype=torch.int64, device=dev) for _ in range(3)]
    expect(step(t, 2, big, hb), PT_ENOTSUP, "PT_COMPLEX", "too large")
    L.pt_trainer_free(t)
    # Adam: the im tables' moments are required; a refused run or step leaves the step count
    t = trainer(_native.PT_ADAM)
    a = _native.AdamState()
    a.ent_m, a.rel_m, a.ent_v, a.rel_v = (moments[i].data_ptr() for i in (0, 1, 4, 5))
    a.beta1, a.beta2, a.eps, a.step = 0.9, 0.999, 1e-8, 7
    expect(L.pt_trainer_set_adam(t, ctypes.byref(a)), PT_EINVAL, "Adam")
    a.ent_transfer_m, a.rel_transfer_m, a.ent_transfer_v, a.rel_transfer_v = (moments[i].data_ptr()
                                                                              for i in (2, 3, 6, 7))
    _native.check(L.pt_trainer_set_adam(t, ctypes.byref(a)))
    expect(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), PT_ENOTSUP, "external batches")
    expect(step(t), PT_ENOTSUP, "PT_COMPLEX", "PT_LOSS_MARGIN")
    assert L.pt_trainer_adam_step(t) == 7
    L.pt_trainer_free(t)
    # universes
    assert L.pt_universe_dim_supported(20, PT) == 0
    job = (_native.UniverseJob * 1)()
    expect(L.pt_universes_train_ex(job, 1, PT, 1, 1, _native.PT_SGD, 0, 1, 0, _native.ptr(losses), st), PT_ENOTSUP,
           "PT_COMPLEX")
    expect(L.pt_universes_train(job, 1, PT, 1, 1, _native.PT_SGD, 0, 1, _native.ptr(losses), st), PT_ENOTSUP,
           "PT_COMPLEX")
    hs = ctypes.c_void_p()
    expect(L.pt_universe_set_create(job, 1, PT, 1, 1, _native.PT_SGD, 0, 1, ctypes.byref(hs)), PT_ENOTSUP, "PT_COMPLEX")
    us = (_native.LpUniverse * 1)()
    pairs = (_native.LpPair * 1)()
    rows = torch.full((E,), 7.0, device=dev)
    expect(L.pt_lp_min_scores(us, 1, PT, 1, 1, pairs, 1, E, _native.ptr(rows), None, st), PT_ENOTSUP, "PT_COMPLEX")
    torch.cuda.synchronize()
    assert (rows == 7.0).all() and (out == 7.0).all() and not losses.any()
    for x, y in zip(tabs, keep):
        assert torch.equal(x, y)
    assert not any(m.any() for m in moments)


def test_steps_timed_covers_both_apply_launches():
    """pt_trainer_steps_timed on a ComplEx trainer: two positive durations, and the steps train all four tables."""
    from openke import _native
    tabs, hrt, cfg = cc.build(cc.ADAGRAD_CASE)
    kge, trn = _trainer(tabs, cfg, "sgd", 0.1)
    trn._setup()
    dev = kge.ent_embeddings.weight.device
    h, t, r = (torch.from_numpy(x).to(dev) for x in hrt)
    loss = torch.zeros(1, device=dev)
    ms2 = (ctypes.c_float * 2)()
    _native.check(_native.lib().pt_trainer_steps_timed(trn._native, cfg["batch_size"], cfg["neg_ent"], _native.ptr(h),
                                                       _native.ptr(t), _native.ptr(r), 3, _native.ptr(loss), ms2,
                                                       _native.stream()))
    assert ms2[0] > 0 and ms2[1] > 0 and np.isfinite(loss.item())
    for a, b in zip(_tables(kge), tabs):
        assert not np.array_equal(a, b)
