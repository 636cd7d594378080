"""DistMult on the GPU (k_step_distmult, k_score_distmult, k_score_queries_distmult: distmult.hip; the L3 form of
k_apply_adam) against the float64 reference tests/distmult_reference.py and the reference implementation's own runs
(tests/golden/distmult_*.npz).

Gradient parity runs SGD at lr 1 on explicit batches (distmult_cases.py), so the table delta is the gradient:
    |delta_gpu - delta_ref64| <= tol = min(1e-5, max(4 * 2^-23 * max(1, |g|max), 4 * GRAD_DEV[family]))
for every cell of both tables, and the loss within min(1e-5, 4 LOSS_DEV) of max(1, |loss|). Scores:
    |got - ref64| <= tol(D) * max(1, |ref64|),  tol(D) = min(1e-5, max(4 * 2^-23, 4 * SCORE_DEV[D])).
The input conditions of the seeds are asserted on the CPU in test_distmult_reference_cpu.py. Every test prints its
observed maxima.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import distmult_cases as dc
import distmult_reference as dr
import oracle
from conftest import KG_SMALL
from helpers import golden, load
from test_distmult_reference_cpu import _margin, lp_excused

pytestmark = pytest.mark.gpu

B1, B2 = 0.9, 0.999
PT_EINVAL, PT_ENOTSUP = 1, 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible HIP device"


def _model(tabs, dim, gamma=None, eps=None):
    from openke.module.model import DistMult
    kge = DistMult(tabs[0].shape[0], tabs[1].shape[0], dim=dim, margin=gamma, epsilon=eps)
    for name, x in zip(dr.TABLES, tabs):
        getattr(kge, name).weight.data.copy_(torch.from_numpy(np.asarray(x)))
    return kge


def _loss(cfg):
    from openke.module.loss import SigmoidLoss, SoftplusLoss
    cls = SigmoidLoss if cfg["loss"] == "sigmoid" else SoftplusLoss
    return cls(adv_temperature=cfg["adv_temperature"])


def _trainer(tabs, cfg, opt, lr):
    """(kge, Trainer) for a DistMult holding the given tables, on the GPU."""
    from openke.config import Trainer
    from openke.module.strategy import NegativeSampling
    kge = _model(tabs, cfg["dim"])
    ns = NegativeSampling(model=kge, loss=_loss(cfg), batch_size=cfg["batch_size"], regul_rate=cfg["regul_rate"],
                          l3_regul_rate=cfg["l3_regul_rate"])
    ns.cuda()
    return kge, Trainer(model=ns, data_loader=None, train_times=0, alpha=lr, use_gpu=True, opt_method=opt)


def _tables(kge):
    return [t.detach().cpu().numpy().copy() for t in kge.tables() if t is not None]


def _check_step(tag, tabs, got, grads, aux, cfg, loss, want_loss, transform=None):
    tol = dr.grad_bound(dr.family(cfg), aux["gmax"])
    devs = []
    for i in range(2):
        want = grads[i] if transform is None else transform(i, grads[i])
        dev = float(np.abs((np.asarray(tabs[i], dtype=np.float64) - got[i].astype(np.float64)) - want).max())
        print("%s %s: max |delta_gpu - delta_ref64| %.3e (tol %.3e, |g|max %.3e)" % (tag, dr.TABLES[i], dev, tol,
                                                                                   aux["gmax"]))
        devs.append(dev)
    print("%s loss gpu %.9g ref %.9g (rel %.3e, tol %.3e)" % (tag, loss, want_loss, abs(loss - want_loss) /
                                                             max(1.0, abs(want_loss)), dr.loss_tol()))
    for i, dev in enumerate(devs):
        assert dev <= tol, (tag, dr.TABLES[i], dev, tol)
    assert dr.loss_close(loss, want_loss), (loss, want_loss)


# ------------------------------------------------------------------ 1. gradient parity ----------
@pytest.mark.parametrize("case", dc.GRAD_CASES + [dc.THRESHOLD_CASE], ids=lambda c: c[0])
def test_gradient_parity_sgd(case):
    tabs, hrt, cfg, mode = dc.build(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = dr.loss_and_grads(tabs, *hrt, bs, cfg, mode)
    kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
    loss = trn.train_one_step(dc.as_batch(hrt, bs, mode))
    got = _tables(kge)
    _check_step(case[0], tabs, got, grads, aux, cfg, loss, want_loss)
    # the entity and the relation no slot names: both rows bit-identical (regul_rate reaches the batch's rows only)
    np.testing.assert_array_equal(got[0][dc.FREE_ENT], tabs[0][dc.FREE_ENT])
    np.testing.assert_array_equal(got[1][dc.FREE_REL], tabs[1][dc.FREE_REL])
    # gradient rows and flags are back to zero: the same step from the same tables gives the same tables and loss
    # to the bound again (a leftover gradient row would double a delta)
    for name, x in zip(dr.TABLES, tabs):
        getattr(kge, name).weight.data.copy_(torch.from_numpy(np.asarray(x)))
    loss2 = trn.train_one_step(dc.as_batch(hrt, bs, mode))
    _check_step(case[0] + " again", tabs, _tables(kge), grads, aux, cfg, loss2, want_loss)


# ------------------------------------------------------------------ 2. Adagrad, Adam -------------
def test_gradient_parity_adagrad_with_regul_rate():
    """The same step through Adagrad (k_apply) from a given state_sum in [1, 2): |d delta / d g| <= 1 there, so the
    gradient bound holds for the delta; both tables and their state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, hrt, cfg, mode = dc.build(dc.ADAGRAD_CASE)
    bs = cfg["batch_size"]
    want_loss, grads, aux = dr.loss_and_grads(tabs, *hrt, bs, cfg, mode)
    kge, trn = _trainer(tabs, cfg, "adagrad", 1.0)
    trn.optimizer = NativeOptimizer(_native.PT_ADAGRAD, 1.0, kge.tables())
    rng = np.random.default_rng(77)
    state = [rng.uniform(1, 2, size=t.shape).astype(np.float32) for t in tabs]
    sums = [s for s in trn.optimizer.state_sum if s is not None]
    assert len(sums) == 2
    for s, x in zip(sums, state):
        s.copy_(torch.from_numpy(x))
    loss = trn.train_one_step(dc.as_batch(hrt, bs, mode))
    got = _tables(kge)
    _check_step("adagrad", tabs, got, grads, aux, cfg, loss, want_loss,
                lambda i, g: g / (np.sqrt(state[i].astype(np.float64) + g ** 2) + 1e-10))
    tol = dr.grad_bound(dr.family(cfg), aux["gmax"])
    for i, s in enumerate(sums):
        dev = float(np.abs(s.cpu().numpy().astype(np.float64) - (state[i].astype(np.float64) + grads[i] ** 2)).max())
        assert dev <= 2.0 ** -22 + 2 * aux["gmax"] * tol, (i, dev)


@pytest.mark.parametrize("case", dc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_three_steps_from_given_state(case):
    """After every step, for both tables: exp_avg / exp_avg_sq within (1 - b1) tol / (1 - b2) 2 |g|max tol of the
    float64 update (gradient with both regularisers) at the GPU's own pre-step state, every weight the float64 update
    formula at the GPU's own new moments (4 ulp of w + 1e-6 |delta|), the loss with the L3 term. Entity 36 and
    relation 2 never occur in a batch and start with zero moments: the bounds above hold for them with the float64
    gradient 3 l3 w |w| alone (asserted nonzero), and with L3 off they stay bit-identical with zero state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, batches, cfg, (m0, v0), lr, step0 = dc.build_adam(case)
    bs, l3 = cfg["batch_size"], cfg["l3_regul_rate"]
    kge, trn = _trainer(tabs, cfg, "adam", lr)
    trn.optimizer = NativeOptimizer(_native.PT_ADAM, lr, kge.tables())
    opt = trn.optimizer
    ms = [x for x in opt.exp_avg if x is not None]
    vs = [x for x in opt.exp_avg_sq if x is not None]
    assert len(ms) == 2 and len(vs) == 2
    for dst, src in zip(ms + vs, m0 + v0):
        dst.copy_(torch.from_numpy(src))
    opt.step = step0

    def state():
        return [x.detach().cpu().numpy().copy() for x in ms], [x.detach().cpu().numpy().copy() for x in vs]

    w = _tables(kge)
    m, v = state()
    free = ((0, dc.FREE_ENT), (1, dc.FREE_REL))
    for s, hrt in enumerate(batches):
        want_loss, grads, aux = dr.loss_and_grads(w, *hrt, bs, cfg)
        for i, row in free:   # the float64 gradient of a never-drawn row is the L3 term alone
            x = w[i][row].astype(np.float64)
            np.testing.assert_allclose(grads[i][row], 3 * l3 * x * np.abs(x), rtol=1e-12, atol=0)
        loss = trn.train_one_step(dc.as_batch(hrt, bs, "normal"))
        assert opt.step == step0 + s + 1
        print("%s step %d loss gpu %.9g ref %.9g" % (case[0], s, loss, want_loss))
        assert dr.loss_close(loss, want_loss), (loss, want_loss)
        w2 = _tables(kge)
        m2, v2 = state()
        tol = dr.grad_bound(dr.family(cfg), aux["gmax"])
        for i in range(2):
            _, mr, vr = dr.adam_update(w[i], m[i], v[i], grads[i], lr, opt.step)
            dm, dv = float(np.abs(m2[i] - mr).max()), float(np.abs(v2[i] - vr).max())
            print("%s step %d %s: |m - ref| %.3e (bound %.3e), |v - ref| %.3e (bound %.3e)"
                  % (case[0], s, dr.TABLES[i], dm, (1 - B1) * tol, dv, (1 - B2) * 2 * aux["gmax"] * tol))
            assert dm <= (1 - B1) * tol
            assert dv <= (1 - B2) * 2 * aux["gmax"] * tol
            wr = dr.adam_weights(w[i], m2[i], v2[i], lr, opt.step)
            bound = 4 * np.spacing(np.abs(w[i])).astype(np.float64) + 1e-6 * np.abs(wr - w[i])
            assert (np.abs(w2[i].astype(np.float64) - wr) <= bound).all(), (case[0], s, i)
        for i, row in free:
            if l3:
                assert (w2[i][row] != w[i][row]).all() and m2[i][row].all() and v2[i][row].all()
            else:
                assert (w2[i][row] == tabs[i][row]).all() and not m2[i][row].any() and not v2[i][row].any()
        w, m, v = w2, m2, v2


# ------------------------------------------------------------------ 3. reference runs ------------
@pytest.mark.parametrize("path", golden("distmult_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_reference_steps_teacher_forced(path):
    """Every recorded step of the reference implementation, from its own tables before the step: the GPU delta within
    the parity bound of the float64 gradient, the loss within the loss bound of float64 and twice that of the recorded
    float32 one."""
    z = load(path)
    cfg = dr.golden_cfg(z)
    bs = cfg["batch_size"]
    for s in range(int(z["steps"])):
        tabs = [np.array(x) for x in dr.golden_tables(z, "s%d" % s)]
        (h, t, r), mode = dr.golden_step(z, cfg, s)
        want_loss, grads, aux = dr.loss_and_grads(tabs, h, t, r, bs, cfg, mode)
        kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
        batch = {"batch_h": z["b%d_h" % s], "batch_t": z["b%d_t" % s], "batch_r": z["b%d_r" % s], "mode": mode}
        loss = trn.train_one_step(batch)
        _check_step("%s step %d" % (path.split("/")[-1], s), tabs, _tables(kge), grads, aux, cfg, loss, want_loss)
        rec = float(z["losses"][s])
        assert abs(loss - rec) <= 2 * dr.loss_tol() * max(1.0, abs(rec)), (loss, rec)


@pytest.mark.parametrize("path", golden("distmult_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_optimizer_runs_match_reference_trajectories(path):
    """The reference implementation's 10-step Adam (with l3_regul_rate) and Adagrad (with regul_rate) runs: losses to
    rtol 1e-4, every table element within the caps of test_gpu_rotate.py's test of the same name. A sanity cap: the
    parity proof is the tests above."""
    z = load(path)
    cfg = dr.golden_cfg(z)
    lr, steps, opt = float(z["lr"]), int(z["steps"]), str(z["optimizer"])
    kge, trn = _trainer([np.array(x) for x in dr.golden_tables(z, "init")], cfg, opt, lr)
    for s in range(steps):
        batch = {"batch_h": z["b%d_h" % s], "batch_t": z["b%d_t" % s], "batch_r": z["b%d_r" % s],
                 "mode": str(z["modes"][s])}
        loss = trn.train_one_step(batch)
        assert abs(loss - float(z["losses"][s])) <= 1e-4 * abs(float(z["losses"][s])), (s, loss, float(z["losses"][s]))
    if opt == "adam":
        assert trn.optimizer.step == steps
    cap = 2 * steps * lr * (1 - B1) / np.sqrt(1 - B2) if opt == "adam" else steps * lr * 1e-3
    for got, want, name in zip(_tables(kge), dr.golden_tables(z, "final"), dr.TABLES):
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


@pytest.mark.parametrize("path", golden("distmult_p*.npz"), ids=lambda p: p.split("/")[-1])
def test_predict_matches_reference(path):
    """predict (-s) in the three modes against the reference implementation's own float32 values; forward is its
    negative."""
    z = load(path)
    D = int(z["dim"])
    kge = _model(dr.golden_tables(z, ""), D, *_margin(z)).cuda()
    tol = dr.score_tol(D if D in dr.SCORE_DEV else 20)
    for mode in ("normal", "head_batch", "tail_batch"):
        data = {"batch_h": z[mode + "_h"], "batch_t": z[mode + "_t"], "batch_r": z[mode + "_r"], "mode": mode}
        got = kge.predict(data).astype(np.float64)
        want = z[mode + "_score"].astype(np.float64)
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print("%s %s: worst %.3e (tol %.3e)" % (path.split("/")[-1], mode, float(err.max()), tol))
        assert (err <= tol).all(), (mode, float(err.max()), tol)
        fwd = kge.forward(data).cpu().numpy()
        np.testing.assert_array_equal(-fwd, kge.predict(data))


@pytest.mark.parametrize("D", dr.SCORE_DIMS)
def test_scores_match_float64(D):
    """pt_score in the three modes (through predict), pt_score_queries and pt_score_rows on both sides, cell by cell."""
    from openke import _native
    L = _native.lib()
    tol = dr.score_tol(D)
    worst = 0.0
    tabs, batches = dr.score_case(D)
    kge = _model(tabs, D).cuda()
    for mode, (h, t, r) in batches.items():
        got = kge.predict({"batch_h": h, "batch_t": t, "batch_r": r, "mode": mode}).astype(np.float64)
        ref = -dr.scores(tabs, *dr.expand_predict(h, t, r, mode), mode)
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert (err <= tol).all(), (D, mode, float(err.max()), tol)
    h, t, r = batches["normal"]
    nq = 5
    for side in (0, 1):
        ref = np.stack([dr.lp_scores(tabs, int(t[i] if side == 0 else h[i]), int(r[i]), side) for i in range(nq)])
        rows = _rows(kge, L.pt_score_rows, side, h[:nq], t[:nq], r[:nq])
        err = np.abs(rows - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert (err <= tol).all(), (D, side, "rows", float(err.max()), tol)
        cand = _rows(kge, L.pt_score_queries, side, h[:nq], t[:nq], r[:nq])
        for i in range(nq):   # candidate order [truth, 0..E-1 without truth]
            truth = int(h[i] if side == 0 else t[i])
            order = oracle.candidates(dr.E, truth)
            np.testing.assert_array_equal(cand[i], rows[i][order])
    print("D %d: worst |gpu - ref64| / max(1, |ref64|) %.3e (tol %.3e)" % (D, worst, tol))


# ------------------------------------------------------------------ 5. link prediction ----------
def test_link_prediction_matches_reference_ranks():
    """Tester.run_link_prediction on kg_small with the recorded tables: every query's raw and filtered rank equal to
    the reference's unless its float64 score vector holds a candidate within 4e-6 relative of the truth; metrics
    equal when no query is excused."""
    from openke.config import Tester
    from openke.data import TestDataLoader
    z = load(golden("distmult_lp.npz")[0])
    tabs = dr.golden_tables(z, "")
    test_dl = TestDataLoader(KG_SMALL, "link")
    kge = _model(tabs, int(z["dim"]), *_margin(z))
    tester = Tester(model=kge, data_loader=test_dl, use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    qs = z["queries"].astype(np.int64)
    h, t, r = test_dl.eval_triples()
    np.testing.assert_array_equal(np.stack([h, t, r], 1), qs)
    excused = lp_excused(tabs, qs)
    assert excused.mean() <= 0.02
    want = z["ranks"].astype(np.int64)
    differ = 0
    for k, g in enumerate(tester.last_ranks):
        d = np.asarray(g, dtype=np.int64) != want[k]
        assert not (d & ~excused[:, k // 2]).any(), (str(z["rank_names"][k]), np.nonzero(d & ~excused[:, k // 2])[0][:10])
        differ += int(d.sum())
    print("distmult_lp: %d ranks differ, %d (query, side) pairs excused" % (differ, int(excused.sum())))
    if not excused.any():
        assert differ == 0
        np.testing.assert_array_equal(np.array(res, dtype=np.float32), z["metrics"].astype(np.float32))


# ------------------------------------------------------------------ 6. example-shaped runs ------
def _example_run(tmp_path, sampling, bern, loss, ns_kw, opt, lr, dim):
    from openke.config import Tester, Trainer
    from openke.data import TestDataLoader, TrainDataLoader
    from openke.module.model import DistMult
    from openke.module.strategy import NegativeSampling
    threads, bs, neg, seed, epochs = 8, 150, 8, 33, 2
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=bs, threads=threads, sampling_mode=sampling, bern_flag=bern,
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
    torch.manual_seed(6)
    kge = DistMult(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=dim)
    ns = NegativeSampling(model=kge, loss=loss, batch_size=dl.get_batch_size(), **ns_kw)
    trn = Trainer(model=ns, data_loader=dl, train_times=epochs, alpha=lr, use_gpu=True, opt_method=opt)
    trn.run()
    assert not trn.last_run_fused
    assert len(trn.epoch_losses) == epochs and np.isfinite(trn.epoch_losses).all()
    assert np.isfinite(trn.last_step_losses).all()
    assert trn.epoch_losses[-1] < trn.epoch_losses[0]
    tester = Tester(model=kge, data_loader=TestDataLoader(KG_SMALL, "link"), use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    assert np.isfinite(np.asarray(res, dtype=np.float64)).all()
    return dl, kge, trn


def test_example_adv_shaped_run_and_checkpoint(tmp_path):
    """Trainer.run() in the shape of examples/train_distmult_WN18_adv.py on kg_small (cross sampling,
    SigmoidLoss(adv_temperature=0.5), l3_regul_rate, Adam) for two epochs, then Tester.run_link_prediction, then
    save_checkpoint -> a fresh DistMult -> load_checkpoint."""
    from openke.module.loss import SigmoidLoss
    from openke.module.model import DistMult
    dl, kge, trn = _example_run(tmp_path, "cross", 0, SigmoidLoss(adv_temperature=0.5), {"l3_regul_rate": 5e-6},
                                "adam", 2e-3, 32)
    assert trn.optimizer.step == 2 * dl.nbatches
    rng = np.random.default_rng(5)
    data = {"batch_h": rng.integers(0, dl.get_ent_tot(), 64), "batch_t": rng.integers(0, dl.get_ent_tot(), 64),
            "batch_r": rng.integers(0, dl.get_rel_tot(), 64), "mode": "normal"}
    before = kge.predict(data)
    path = os.path.join(str(tmp_path), "distmult.ckpt")
    kge.save_checkpoint(path)
    torch.manual_seed(99)
    fresh = DistMult(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=32).cuda()
    assert not np.array_equal(fresh.predict(data), before)
    fresh.load_checkpoint(path)
    np.testing.assert_array_equal(fresh.predict(data), before)


def test_example_softplus_shaped_run(tmp_path):
    """Trainer.run() in the shape of examples/train_distmult_WN18.py on kg_small (normal sampling with bern,
    SoftplusLoss, regul_rate 1, Adagrad) for two epochs."""
    from openke.module.loss import SoftplusLoss
    _example_run(tmp_path, "normal", 1, SoftplusLoss(), {"regul_rate": 1.0}, "adagrad", 0.5, 20)


# ------------------------------------------------------------------ 7. refusals -----------------
def test_unsupported_python_combinations_raise():
    """deterministic=True, MarginLoss, L3 without Adam and a universe configuration with DistMult; regul_rate on TransE
    and RotatE as before: NotImplementedError by name, the tables untouched."""
    from openke.config import Parallel_Universe_Config, Trainer
    from openke.module.loss import MarginLoss, SigmoidLoss, SoftplusLoss
    from openke.module.model import DistMult, RotatE, TransE
    from openke.module.strategy import NegativeSampling
    batch = {"batch_h": np.array([0, 1, 2, 3]), "batch_t": np.array([1, 2, 3, 4]), "batch_r": np.array([0, 1, 0, 1]),
             "mode": "normal"}
    cases = [
        (DistMult, SigmoidLoss(adv_temperature=2), {}, {"deterministic": True}, "not implemented for DistMult"),
        (DistMult, MarginLoss(margin=1.0), {}, {}, "MarginLoss on DistMult"),
        (DistMult, SoftplusLoss(), {"l3_regul_rate": 0.1}, {"opt_method": "sgd"}, "l3_regul_rate"),
        (DistMult, SigmoidLoss(), {"l3_regul_rate": 0.1}, {"opt_method": "adagrad"}, "l3_regul_rate"),
        (TransE, MarginLoss(margin=1.0), {"regul_rate": 0.1}, {}, "regularisation"),
        (TransE, SigmoidLoss(), {"l3_regul_rate": 0.1}, {"opt_method": "adam"}, "regularisation"),
        (RotatE, SigmoidLoss(adv_temperature=2), {"regul_rate": 0.1}, {}, "regularisation"),
        (RotatE, SigmoidLoss(), {"l3_regul_rate": 0.1}, {"opt_method": "adam"}, "regularisation"),
        (TransE, SoftplusLoss(), {}, {}, "SoftplusLoss"),
    ]
    for cls, loss, ns_kw, tr_kw, frag in cases:
        torch.manual_seed(1)
        kge = cls(6, 2, dim=8)
        ns = NegativeSampling(model=kge, loss=loss, batch_size=2, **ns_kw)
        w0 = [t.detach().clone() for t in kge.tables() if t is not None]
        trn = Trainer(model=ns, data_loader=None, train_times=0, alpha=0.1, use_gpu=True, **tr_kw)
        with pytest.raises(NotImplementedError, match=frag):
            trn.train_one_step(batch)
        for a, b in zip(w0, [t for t in kge.tables() if t is not None]):
            assert torch.equal(a, b.detach().cpu())
    pu = object.__new__(Parallel_Universe_Config)
    pu.embedding_model = DistMult
    with pytest.raises(NotImplementedError, match="DistMult"):
        pu._check_setup()


def test_unsupported_native_combinations_are_refused():
    """Every PT_DISTMULT refusal of the C ABI: PT_ENOTSUP / PT_EINVAL with a message that names the model, rows,
    moments and the Adam step count untouched."""
    from openke import _native
    from openke.data import TrainDataLoader
    L = _native.lib()
    dev = torch.device("cuda", 0)
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=50, threads=8, bern_flag=0, filter_flag=1, neg_ent=2,
                         random_seed=3)
    sampler = dl.device_sampler()
    E, R, D = dl.get_ent_tot(), dl.get_rel_tot(), 8
    tabs = [torch.rand(E, D, device=dev) - 0.5, torch.rand(R, D, device=dev) - 0.5]
    keep = [x.clone() for x in tabs]
    moments = [torch.zeros_like(x) for x in tabs + tabs]
    losses = torch.zeros(4, device=dev)
    st = _native.stream()

    def desc(opt, model=_native.PT_DISTMULT):
        d = _native.ModelDesc()
        d.model, d.p_norm, d.norm_flag, d.opt, d.lr, d.margin = model, 1, 0, opt, 0.1, 2.0
        d.ent_total, d.rel_total, d.dim = E, R, D
        d.ent, d.rel = tabs[0].data_ptr(), tabs[1].data_ptr()
        return d

    def trainer(opt, model=_native.PT_DISTMULT):
        h = ctypes.c_void_p()
        d = desc(opt, model)
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
    # the dim rule is TransE's; the query answers 0 for the id
    for dim, ok in ((1, True), (511, True), (513, False), (516, True), (1024, True), (1028, False)):
        assert L.pt_model_dim_supported(dim, _native.PT_DISTMULT) == 0
        wide = [torch.zeros(4, dim, device=dev), torch.zeros(2, dim, device=dev)]
        d = desc(_native.PT_SGD)
        d.p_norm = 7   # (not read)
        d.ent_total, d.rel_total, d.dim, d.ent, d.rel = 4, 2, dim, wide[0].data_ptr(), wide[1].data_ptr()
        if ok:
            _native.check(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)))
            L.pt_trainer_free(h)
        else:
            expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), PT_ENOTSUP, "DistMult", str(dim))
    b = [torch.zeros(50 * 3, dtype=torch.int64, device=dev) for _ in range(3)]

    def step(t, bs=50, neg=2, arrays=b):
        return L.pt_trainer_step(t, None, bs, neg, 0, 0, _native.ptr(arrays[0]), _native.ptr(arrays[1]),
                                 _native.ptr(arrays[2]), _native.ptr(losses), st)

    # SGD trainer: no captured run, no in-kernel sampling, no timed run, no reference-order mode
    t = trainer(_native.PT_SGD)
    ms4 = (ctypes.c_float * 4)()
    expect(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), PT_ENOTSUP, "PT_DISTMULT",
           "external batches")
    expect(L.pt_trainer_step(t, sampler, 50, 2, 0, 1, None, None, None, _native.ptr(losses), st), PT_ENOTSUP,
           "PT_DISTMULT")
    expect(L.pt_trainer_run_timed(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), ms4, st), PT_ENOTSUP, "PT_DISTMULT")
    expect(L.pt_trainer_set_deterministic(t, 1), PT_ENOTSUP, "PT_DISTMULT")
    # no loss set (the default is the margin loss), PT_LOSS_MARGIN, a model margin
    expect(step(t), PT_ENOTSUP, "PT_DISTMULT", "PT_LOSS_MARGIN")
    ld = loss_desc(_native.PT_LOSS_MARGIN, 1, 0)
    expect(L.pt_trainer_set_loss(t, ctypes.byref(ld)), PT_ENOTSUP, "PT_DISTMULT", "PT_LOSS_MARGIN")
    ld = loss_desc(_native.PT_LOSS_SIGMOID, 1, 1)
    expect(L.pt_trainer_set_loss(t, ctypes.byref(ld)), PT_ENOTSUP, "PT_DISTMULT", "score_margin_flag")
    ld = loss_desc(_native.PT_LOSS_SIGMOID, 1, 0)
    _native.check(L.pt_trainer_set_loss(t, ctypes.byref(ld)))
    # the regulariser descriptor
    for rd in (regul(-1.0, 0.0, 0), regul(float("nan"), 0.0, 0), regul(0.0, float("inf"), 0), regul(0.0, -1e-3, 0)):
        expect(L.pt_trainer_set_regul(t, ctypes.byref(rd)), PT_EINVAL, "regul_rate")
    for mode in (-1, 3):
        rd = regul(1.0, 0.0, mode)
        expect(L.pt_trainer_set_regul(t, ctypes.byref(rd)), PT_EINVAL, "batch_mode")
    expect(L.pt_trainer_set_regul(t, None), PT_EINVAL)
    # L3 under SGD: refused at the step
    rd = regul(1.0, 1e-3, 2)
    _native.check(L.pt_trainer_set_regul(t, ctypes.byref(rd)))
    expect(step(t), PT_ENOTSUP, "PT_DISTMULT", "l3_regul_rate")
    rd = regul(0.0, 0.0, 0)
    _native.check(L.pt_trainer_set_regul(t, ctypes.byref(rd)))
    # neg past the LDS score buffer
    big = 16384
    hb = [torch.zeros(2 * (big + 1), dtype=torch.int64, device=dev) for _ in range(3)]
    expect(step(t, 2, big, hb), PT_ENOTSUP, "PT_DISTMULT", "too large")
    L.pt_trainer_free(t)
    # a nonzero rate on another model; zero rates pass
    for model in (_native.PT_TRANSE, _native.PT_ROTATE):
        wide = [torch.zeros(E, 2 * D, device=dev), torch.zeros(R, D, device=dev)]
        d = desc(_native.PT_SGD, model)
        d.phase_div = 0.5
        if model == _native.PT_ROTATE:
            d.ent = wide[0].data_ptr()
        _native.check(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)))
        for rd in (regul(0.5, 0.0, 0), regul(0.0, 0.5, 0)):
            expect(L.pt_trainer_set_regul(h, ctypes.byref(rd)), PT_ENOTSUP, "PT_DISTMULT")
        rd = regul(0.0, 0.0, 1)
        _native.check(L.pt_trainer_set_regul(h, ctypes.byref(rd)))
        L.pt_trainer_free(h)
    # Adam: a refused run or step leaves the step count
    t = trainer(_native.PT_ADAM)
    a = _native.AdamState()
    a.ent_m, a.rel_m, a.ent_v, a.rel_v = (x.data_ptr() for x in moments)
    a.beta1, a.beta2, a.eps, a.step = 0.9, 0.999, 1e-8, 7
    _native.check(L.pt_trainer_set_adam(t, ctypes.byref(a)))
    expect(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), PT_ENOTSUP, "external batches")
    expect(step(t), PT_ENOTSUP, "PT_DISTMULT", "PT_LOSS_MARGIN")
    assert L.pt_trainer_adam_step(t) == 7
    L.pt_trainer_free(t)
    # universes
    assert L.pt_universe_dim_supported(20, _native.PT_DISTMULT) == 0
    job = (_native.UniverseJob * 1)()
    expect(L.pt_universes_train_ex(job, 1, _native.PT_DISTMULT, 1, 1, _native.PT_SGD, 0, 1, 0, _native.ptr(losses),
                                   st), PT_ENOTSUP, "PT_DISTMULT")
    expect(L.pt_universes_train(job, 1, _native.PT_DISTMULT, 1, 1, _native.PT_SGD, 0, 1, _native.ptr(losses), st),
           PT_ENOTSUP, "PT_DISTMULT")
    hs = ctypes.c_void_p()
    expect(L.pt_universe_set_create(job, 1, _native.PT_DISTMULT, 1, 1, _native.PT_SGD, 0, 1, ctypes.byref(hs)),
           PT_ENOTSUP, "PT_DISTMULT")
    us = (_native.LpUniverse * 1)()
    pairs = (_native.LpPair * 1)()
    rows = torch.full((E,), 7.0, device=dev)
    expect(L.pt_lp_min_scores(us, 1, _native.PT_DISTMULT, 1, 1, pairs, 1, E, _native.ptr(rows), None, st), PT_ENOTSUP,
           "PT_DISTMULT")
    torch.cuda.synchronize()
    assert (rows == 7.0).all() and not losses.any()
    for x, y in zip(tabs, keep):
        assert torch.equal(x, y)
    assert not any(m.any() for m in moments)
