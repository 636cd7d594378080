"""RotatE on the GPU (k_step_rotate, k_score_rotate, k_score_queries_rotate; rotate.hip) against the float64 reference
tests/rotate_reference.py and the reference implementation's own runs (tests/golden/rotate_*.npz).

Gradient parity runs SGD at lr 1 on explicit batches (rotate_cases.py), so the table delta is the gradient:
    |delta_gpu - delta_ref64| <= tol = min(1e-5, max(4 * 2^-23 * max(1, |g|max), 4 * GRAD_DEV[family]))
for every cell of both tables (test_gpu_adv.py's bound and reasons), and the loss to rtol 1e-5 of max(1, |loss|).
Scores:
    |got - ref64| <= tol(D) * max(1, ref64),  tol(D) = min(1e-5, max(4 * 2^-23, 4 * SCORE_DEV[D]))
(test_gpu_lp_values.py's rule). The input conditions of the seeds are asserted on the CPU in
test_rotate_reference_cpu.py. Every test prints its observed maxima.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
import rotate_cases as rc
import rotate_reference as rr
from conftest import KG_SMALL
from helpers import golden, load
from test_rotate_reference_cpu import lp_excused

pytestmark = pytest.mark.gpu

B1, B2 = 0.9, 0.999
PT_EINVAL, PT_ENOTSUP = 1, 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible HIP device"


def _model(tabs, dim, gamma=rc.GAMMA, eps=rc.EPS):
    from openke.module.model import RotatE
    kge = RotatE(tabs[0].shape[0], tabs[1].shape[0], dim=dim, margin=gamma, epsilon=eps)
    for name, x in zip(rr.TABLES, tabs):
        getattr(kge, name).weight.data.copy_(torch.from_numpy(np.asarray(x)))
    return kge


def _loss(cfg):
    from openke.module.loss import MarginLoss, SigmoidLoss
    if cfg["loss"] == "sigmoid":
        return SigmoidLoss(adv_temperature=cfg["adv_temperature"])
    return MarginLoss(adv_temperature=cfg["adv_temperature"], margin=cfg["loss_margin"])


def _trainer(tabs, cfg, opt, lr):
    """(kge, Trainer) for a RotatE holding the given tables, on the GPU."""
    from openke.config import Trainer
    from openke.module.strategy import NegativeSampling
    kge = _model(tabs, cfg["dim"], cfg["model_margin"], cfg["epsilon"])
    assert kge.phase_divisor() == cfg["phase_div"]
    ns = NegativeSampling(model=kge, loss=_loss(cfg), batch_size=cfg["batch_size"])
    ns.cuda()
    return kge, Trainer(model=ns, data_loader=None, train_times=0, alpha=lr, use_gpu=True, opt_method=opt)


def _tables(kge):
    return [t.detach().cpu().numpy().copy() for t in kge.tables() if t is not None]


def _loss_close(loss, want):
    return abs(loss - want) <= 1e-5 * max(1.0, abs(want))


def _check_step(tag, tabs, got, grads, aux, cfg, loss, want_loss, transform=None):
    tol = rr.grad_bound(rr.family(cfg), aux["gmax"])
    devs = []
    for i in range(2):
        want = grads[i] if transform is None else transform(i, grads[i])
        dev = float(np.abs((np.asarray(tabs[i], dtype=np.float64) - got[i].astype(np.float64)) - want).max())
        print("%s %s: max |delta_gpu - delta_ref64| %.3e (tol %.3e, |g|max %.3e)" % (tag, rr.TABLES[i], dev, tol,
                                                                                   aux["gmax"]))
        devs.append(dev)
    print("%s loss gpu %.9g ref %.9g" % (tag, loss, want_loss))
    for i, dev in enumerate(devs):
        assert dev <= tol, (tag, rr.TABLES[i], dev, tol)
    assert _loss_close(loss, want_loss), (loss, want_loss)


# ------------------------------------------------------------------ 1. gradient parity ----------
@pytest.mark.parametrize("case", rc.GRAD_CASES, ids=lambda c: c[0])
def test_gradient_parity_sgd(case):
    tabs, hrt, cfg, mode = rc.build(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    flags = rc.planted(*hrt, bs, K, mode)
    assert all(v for k, v in flags.items() if k != "other_relation") and flags["other_relation"] == (mode == "normal")
    want_loss, grads, aux = rr.loss_and_grads(tabs, *hrt, bs, cfg, mode)
    kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
    loss = trn.train_one_step(rc.as_batch(hrt, bs, mode))
    got = _tables(kge)
    _check_step(case[0], tabs, got, grads, aux, cfg, loss, want_loss)
    # the entity and the relation no slot names: both rows bit-identical
    np.testing.assert_array_equal(got[0][rc.FREE_ENT], tabs[0][rc.FREE_ENT])
    np.testing.assert_array_equal(got[1][rc.FREE_REL], tabs[1][rc.FREE_REL])


# ------------------------------------------------------------------ 2. Adagrad, Adam -------------
def test_gradient_parity_adagrad():
    """The same step through Adagrad (k_apply on the half-row view) from a given state_sum in [1, 2):
    |d delta / d g| <= 1 there, so the gradient bound holds for the delta; both tables and their state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    case = rc.ADAGRAD_CASE
    tabs, hrt, cfg, mode = rc.build(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = rr.loss_and_grads(tabs, *hrt, bs, cfg, mode)
    kge, trn = _trainer(tabs, cfg, "adagrad", 1.0)
    trn.optimizer = NativeOptimizer(_native.PT_ADAGRAD, 1.0, kge.tables())
    rng = np.random.default_rng(77)
    state = [rng.uniform(1, 2, size=t.shape).astype(np.float32) for t in tabs]
    sums = [s for s in trn.optimizer.state_sum if s is not None]
    assert len(sums) == 2
    for s, x in zip(sums, state):
        s.copy_(torch.from_numpy(x))
    loss = trn.train_one_step(rc.as_batch(hrt, bs, mode))
    got = _tables(kge)
    _check_step("adagrad", tabs, got, grads, aux, cfg, loss, want_loss,
                lambda i, g: g / (np.sqrt(state[i].astype(np.float64) + g ** 2) + 1e-10))
    tol = rr.grad_bound(rr.family(cfg), aux["gmax"])
    for i, s in enumerate(sums):
        dev = float(np.abs(s.cpu().numpy().astype(np.float64) - (state[i].astype(np.float64) + grads[i] ** 2)).max())
        assert dev <= 2.0 ** -22 + 2 * aux["gmax"] * tol, (i, dev)


@pytest.mark.parametrize("case", rc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_three_steps_from_given_state(case):
    """After every step, for both tables: exp_avg / exp_avg_sq within (1 - b1) tol / (1 - b2) 2 |g|max tol of the
    float64 update at the GPU's own pre-step state, every weight the float64 update formula at the GPU's own new
    moments (4 ulp of w + 1e-6 |delta|); the row touched in step 1 only keeps moving, the row never touched stays put
    with zero state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, batches, cfg, (m0, v0), lr, step0 = rc.build_adam(case)
    bs = cfg["batch_size"]
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
    once, free = rc.ONCE_ENT, rc.FREE_ENT
    for s, hrt in enumerate(batches):
        want_loss, grads, aux = rr.loss_and_grads(w, *hrt, bs, cfg)
        loss = trn.train_one_step(rc.as_batch(hrt, bs, "normal"))
        assert opt.step == step0 + s + 1
        assert _loss_close(loss, want_loss), (loss, want_loss)
        w2 = _tables(kge)
        m2, v2 = state()
        tol = rr.grad_bound(rr.family(cfg), aux["gmax"])
        for i in range(2):
            _, mr, vr = rr.adam_update(w[i], m[i], v[i], grads[i], lr, opt.step)
            dm, dv = float(np.abs(m2[i] - mr).max()), float(np.abs(v2[i] - vr).max())
            print("%s step %d %s: |m - ref| %.3e (bound %.3e), |v - ref| %.3e (bound %.3e)"
                  % (case[0], s, rr.TABLES[i], dm, (1 - B1) * tol, dv, (1 - B2) * 2 * aux["gmax"] * tol))
            assert dm <= (1 - B1) * tol
            assert dv <= (1 - B2) * 2 * aux["gmax"] * tol
            wr = rr.adam_weights(w[i], m2[i], v2[i], lr, opt.step)
            bound = 4 * np.spacing(np.abs(w[i])).astype(np.float64) + 1e-6 * np.abs(wr - w[i])
            assert (np.abs(w2[i].astype(np.float64) - wr) <= bound).all(), (case[0], s, i)
        # entity 35: touched in step 1 only, still moving; entity 36: never touched
        assert (w2[0][once] != w[0][once]).any(), "row %d must move in step %d" % (once, s + 1)
        assert (grads[0][once] != 0).any() == (s == 0)
        assert (w2[0][free] == tabs[0][free]).all() and not m2[0][free].any() and not v2[0][free].any()
        w, m, v = w2, m2, v2


# ------------------------------------------------------------------ 3. reference runs ------------
@pytest.mark.parametrize("path", golden("rotate_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_reference_steps_teacher_forced(path):
    """Every recorded step of the reference implementation, from its own tables before the step: the GPU delta within
    the parity bound of the float64 gradient, the loss to rtol 1e-5 of float64 and of the recorded one."""
    z = load(path)
    cfg = rr.golden_cfg(z)
    bs = cfg["batch_size"]
    for s in range(int(z["steps"])):
        tabs = [np.array(x) for x in rr.golden_tables(z, "s%d" % s)]
        (h, t, r), mode = rr.golden_step(z, cfg, s)
        want_loss, grads, aux = rr.loss_and_grads(tabs, h, t, r, bs, cfg, mode)
        kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
        batch = {"batch_h": z["b%d_h" % s], "batch_t": z["b%d_t" % s], "batch_r": z["b%d_r" % s], "mode": mode}
        loss = trn.train_one_step(batch)
        _check_step("%s step %d" % (path.split("/")[-1], s), tabs, _tables(kge), grads, aux, cfg, loss, want_loss)
        assert _loss_close(loss, float(z["losses"][s]))


@pytest.mark.parametrize("path", golden("rotate_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_optimizer_runs_match_reference_trajectories(path):
    """The reference implementation's 10-step Adam and Adagrad runs: losses to rtol 1e-4, every table element within
    the caps of test_gpu_transd.py's test of the same name (Adam's per-step bound for two trajectories; Adagrad steps
    * lr * 1e-3). A sanity cap: the parity proof is the tests above."""
    z = load(path)
    cfg = rr.golden_cfg(z)
    lr, steps, opt = float(z["lr"]), int(z["steps"]), str(z["optimizer"])
    kge, trn = _trainer([np.array(x) for x in rr.golden_tables(z, "init")], cfg, opt, lr)
    for s in range(steps):
        batch = {"batch_h": z["b%d_h" % s], "batch_t": z["b%d_t" % s], "batch_r": z["b%d_r" % s],
                 "mode": str(z["modes"][s])}
        loss = trn.train_one_step(batch)
        assert abs(loss - float(z["losses"][s])) <= 1e-4 * abs(float(z["losses"][s])), (s, loss, float(z["losses"][s]))
    if opt == "adam":
        assert trn.optimizer.step == steps
    cap = 2 * steps * lr * (1 - B1) / np.sqrt(1 - B2) if opt == "adam" else steps * lr * 1e-3
    for got, want, name in zip(_tables(kge), rr.golden_tables(z, "final"), rr.TABLES):
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


@pytest.mark.parametrize("path", golden("rotate_p*.npz"), ids=lambda p: p.split("/")[-1])
def test_predict_matches_reference(path):
    """predict (distance - margin) in the three modes against the reference implementation's own float32 values."""
    z = load(path)
    D, gamma = int(z["dim"]), float(z["model_margin"])
    kge = _model(rr.golden_tables(z, ""), D, gamma, float(z["epsilon"])).cuda()
    assert kge.phase_divisor() == rr.phase_div(float(z["rel_embedding_range"]))
    tol = rr.score_tol(D if D in rr.SCORE_DEV else 20)
    for mode in ("normal", "head_batch", "tail_batch"):
        data = {"batch_h": z[mode + "_h"], "batch_t": z[mode + "_t"], "batch_r": z[mode + "_r"], "mode": mode}
        got = kge.predict(data).astype(np.float64)
        want = z[mode + "_score"].astype(np.float64)
        # a score cell is the distance: predict = d - gamma, the bound is relative to max(1, d)
        err = np.abs(got - want) / np.maximum(1.0, want + gamma)
        print("%s %s: worst %.3e (tol %.3e)" % (path.split("/")[-1], mode, float(err.max()), tol))
        assert (err <= tol).all(), (mode, float(err.max()), tol)
        fwd = kge.forward(data).cpu().numpy()
        np.testing.assert_array_equal(-fwd, kge.predict(data))


@pytest.mark.parametrize("D", rr.SCORE_DIMS)
def test_scores_match_float64(D):
    """pt_score in the three modes (through predict), pt_score_queries and pt_score_rows on both sides; head_batch
    equals tail_batch on the same triples within the tolerance."""
    from openke import _native
    L = _native.lib()
    tol = rr.score_tol(D)
    worst = 0.0
    tabs, batches, q = rr.score_case(D)
    kge = _model(tabs, D, rr.SCORE_GAMMA, rr.SCORE_EPS).cuda()
    assert kge.phase_divisor() == q
    gamma = rr.SCORE_GAMMA
    for mode, (h, t, r) in batches.items():
        got = kge.predict({"batch_h": h, "batch_t": t, "batch_r": r, "mode": mode}).astype(np.float64) + gamma
        ref = rr.scores(tabs, *rr.expand_predict(h, t, r, mode), q, mode)
        err = np.abs(got - ref) / np.maximum(1.0, ref)
        worst = max(worst, float(err.max()))
        assert (err <= tol).all(), (D, mode, float(err.max()), tol)
    # one fixed tail and relation, the heads varying (head_batch) against the same triples given as a tail_batch each
    h, t, r = batches["head_batch"]
    hb = kge.predict({"batch_h": h, "batch_t": t, "batch_r": r, "mode": "head_batch"}).astype(np.float64) + gamma
    tb = np.array([kge.predict({"batch_h": h[i:i + 1], "batch_t": t, "batch_r": r, "mode": "tail_batch"})[0]
                   for i in range(8)], dtype=np.float64) + gamma
    err = np.abs(hb[:8] - tb) / np.maximum(1.0, tb)
    assert (err <= 2 * tol).all(), (D, "head vs tail", float(err.max()))
    h, t, r = batches["normal"]
    nq = 5
    for side in (0, 1):
        ref = np.stack([rr.lp_scores(tabs, int(t[i] if side == 0 else h[i]), int(r[i]), side, q) for i in range(nq)])
        rows = _rows(kge, L.pt_score_rows, side, h[:nq], t[:nq], r[:nq])
        err = np.abs(rows - ref) / np.maximum(1.0, ref)
        worst = max(worst, float(err.max()))
        assert (err <= tol).all(), (D, side, "rows", float(err.max()), tol)
        cand = _rows(kge, L.pt_score_queries, side, h[:nq], t[:nq], r[:nq])
        for i in range(nq):   # candidate order [truth, 0..E-1 without truth]
            truth = int(h[i] if side == 0 else t[i])
            order = oracle.candidates(rr.E, truth)
            np.testing.assert_array_equal(cand[i], rows[i][order])
    print("D %d: worst |gpu - ref64| / max(1, ref64) %.3e (tol %.3e)" % (D, worst, tol))


# ------------------------------------------------------------------ 5. link prediction ----------
def test_link_prediction_matches_reference_ranks():
    """Tester.run_link_prediction on kg_small with the recorded tables: every query's raw and filtered rank equal to
    the reference's unless its float64 score vector holds a candidate within 4e-6 relative of the truth; metrics
    equal when no query is excused."""
    from openke.config import Tester
    from openke.data import TestDataLoader
    z = load(golden("rotate_lp.npz")[0])
    tabs = rr.golden_tables(z, "")
    q = rr.phase_div(float(z["rel_embedding_range"]))
    test_dl = TestDataLoader(KG_SMALL, "link")
    kge = _model(tabs, int(z["dim"]), float(z["model_margin"]), float(z["epsilon"]))
    tester = Tester(model=kge, data_loader=test_dl, use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    qs = z["queries"].astype(np.int64)
    h, t, r = test_dl.eval_triples()
    np.testing.assert_array_equal(np.stack([h, t, r], 1), qs)
    excused = lp_excused(tabs, qs, q)
    assert excused.any(axis=0).mean() <= 0.02
    want = z["ranks"].astype(np.int64)
    differ = 0
    for k, g in enumerate(tester.last_ranks):
        d = np.asarray(g, dtype=np.int64) != want[k]
        assert not (d & ~excused[k // 2]).any(), (str(z["rank_names"][k]), np.nonzero(d & ~excused[k // 2])[0][:10])
        differ += int(d.sum())
    print("rotate_lp: %d ranks differ, %d (query, side) pairs excused" % (differ, int(excused.sum())))
    if not excused.any():
        assert differ == 0
        np.testing.assert_array_equal(np.array(res, dtype=np.float32), z["metrics"].astype(np.float32))


# ------------------------------------------------------------------ 6. example-shaped run -------
def test_example_shaped_run_link_prediction_and_checkpoint(tmp_path):
    """Trainer.run() in the shape of examples/train_rotate_WN18_adv.py on kg_small (cross sampling,
    SigmoidLoss(adv_temperature=2), Adam), then Tester.run_link_prediction, then save_checkpoint -> a fresh RotatE ->
    load_checkpoint."""
    from openke.config import Tester, Trainer
    from openke.data import TestDataLoader, TrainDataLoader
    from openke.module.loss import SigmoidLoss
    from openke.module.model import RotatE
    from openke.module.strategy import NegativeSampling
    threads, bs, neg, seed, epochs = 8, 150, 8, 33, 4
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=bs, threads=threads, sampling_mode="cross", bern_flag=0,
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
    torch.manual_seed(6)
    kge = RotatE(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=32, margin=6.0, epsilon=2.0)
    ns = NegativeSampling(model=kge, loss=SigmoidLoss(adv_temperature=2), batch_size=dl.get_batch_size(),
                          regul_rate=0.0)
    trn = Trainer(model=ns, data_loader=dl, train_times=epochs, alpha=2e-3, use_gpu=True, opt_method="adam")
    trn.run()
    assert not trn.last_run_fused
    assert len(trn.epoch_losses) == epochs and np.isfinite(trn.epoch_losses).all()
    assert np.isfinite(trn.last_step_losses).all()
    assert trn.epoch_losses[-1] < trn.epoch_losses[0]
    assert trn.optimizer.step == epochs * dl.nbatches
    tester = Tester(model=kge, data_loader=TestDataLoader(KG_SMALL, "link"), use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    assert np.isfinite(np.asarray(res, dtype=np.float64)).all()
    rng = np.random.default_rng(5)
    data = {"batch_h": rng.integers(0, dl.get_ent_tot(), 64), "batch_t": rng.integers(0, dl.get_ent_tot(), 64),
            "batch_r": rng.integers(0, dl.get_rel_tot(), 64), "mode": "normal"}
    before = kge.predict(data)
    path = os.path.join(str(tmp_path), "rotate.ckpt")
    kge.save_checkpoint(path)
    torch.manual_seed(99)
    fresh = RotatE(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=32, margin=6.0, epsilon=2.0).cuda()
    assert not np.array_equal(fresh.predict(data), before)
    fresh.load_checkpoint(path)
    np.testing.assert_array_equal(fresh.predict(data), before)


# ------------------------------------------------------------------ 7. initial tables -----------
@pytest.mark.parametrize("path", golden("rotate_g[12].npz") + golden("rotate_p1.npz") + golden("rotate_lp.npz"),
                         ids=lambda p: p.split("/")[-1])
def test_seeded_construction_gives_the_reference_tables(path):
    from openke.module.model import RotatE
    z = load(path)
    ent0, rel0 = rr.golden_tables(z, "init")
    torch.manual_seed(int(z["torch_seed"]))
    kge = RotatE(ent0.shape[0], rel0.shape[0], dim=int(z["dim"]), margin=float(z["model_margin"]),
                 epsilon=float(z["epsilon"]))
    np.testing.assert_array_equal(kge.ent_embeddings.weight.detach().numpy(), ent0)
    np.testing.assert_array_equal(kge.rel_embeddings.weight.detach().numpy(), rel0)
    assert sorted(kge.state_dict().keys()) == [str(k) for k in z["state_keys"]]
    assert kge.rel_embedding_range.item() == float(z["rel_embedding_range"])
    kge.cuda()   # the divisor is formed on the CPU whatever the device
    assert kge.phase_divisor() == rr.phase_div(float(z["rel_embedding_range"]))


# ------------------------------------------------------------------ 8. refusals -----------------
def test_unsupported_python_combinations_raise():
    """deterministic=True, regularisation and a universe configuration with RotatE: NotImplementedError by name, the
    tables untouched."""
    from openke.config import Parallel_Universe_Config, Trainer
    from openke.module.loss import MarginLoss, SigmoidLoss
    from openke.module.model import RotatE
    from openke.module.strategy import NegativeSampling
    batch = {"batch_h": np.array([0, 1, 2, 3]), "batch_t": np.array([1, 2, 3, 4]), "batch_r": np.array([0, 1, 0, 1]),
             "mode": "normal"}
    cases = [
        (SigmoidLoss(adv_temperature=2), {}, {"deterministic": True}, "not implemented for RotatE"),
        (MarginLoss(margin=1.0), {}, {"deterministic": True}, "not implemented for RotatE"),
        (SigmoidLoss(adv_temperature=2), {"regul_rate": 0.1}, {}, "regularisation"),
        (SigmoidLoss(), {"l3_regul_rate": 0.1}, {}, "regularisation"),
    ]
    for loss, ns_kw, tr_kw, frag in cases:
        torch.manual_seed(1)
        kge = RotatE(6, 2, dim=8)
        ns = NegativeSampling(model=kge, loss=loss, batch_size=2, **ns_kw)
        w0 = [t.detach().clone() for t in kge.tables() if t is not None]
        trn = Trainer(model=ns, data_loader=None, train_times=0, alpha=0.1, use_gpu=True, **tr_kw)
        with pytest.raises(NotImplementedError, match=frag):
            trn.train_one_step(batch)
        for a, b in zip(w0, [t for t in kge.tables() if t is not None]):
            assert torch.equal(a, b.detach().cpu())
    pu = object.__new__(Parallel_Universe_Config)
    pu.embedding_model = RotatE
    with pytest.raises(NotImplementedError, match="RotatE"):
        pu._check_setup()


def test_unsupported_native_combinations_are_refused():
    """Every PT_ROTATE refusal of the C ABI: PT_ENOTSUP / PT_EINVAL with a message, rows, moments and the Adam step
    count untouched."""
    from openke import _native
    from openke.data import TrainDataLoader
    L = _native.lib()
    dev = torch.device("cuda", 0)
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=50, threads=8, bern_flag=0, filter_flag=1, neg_ent=2,
                         random_seed=3)
    sampler = dl.device_sampler()
    E, R, D = dl.get_ent_tot(), dl.get_rel_tot(), 8
    tabs = [torch.rand(E, 2 * D, device=dev) - 0.5, torch.rand(R, D, device=dev) - 0.5]
    keep = [x.clone() for x in tabs]
    moments = [torch.zeros_like(x) for x in tabs + tabs]
    losses = torch.zeros(4, device=dev)
    st = _native.stream()

    def desc(opt, q=0.5):
        d = _native.ModelDesc()
        d.model, d.p_norm, d.norm_flag, d.opt, d.lr, d.margin = _native.PT_ROTATE, 1, 0, opt, 0.1, 2.0
        d.ent_total, d.rel_total, d.dim = E, R, D
        d.ent, d.rel = tabs[0].data_ptr(), tabs[1].data_ptr()
        d.phase_div = q
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

    assert L.pt_version() == 1
    # the descriptor: a finite positive phase divisor; the dim rule is TransE's
    h = ctypes.c_void_p()
    for q in (0.0, -1.0, float("inf"), float("nan")):
        d = desc(_native.PT_SGD, q)
        expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), PT_EINVAL, "PT_ROTATE", "phase divisor")
    for dim, ok in ((1, True), (511, True), (513, False), (516, True), (1024, True), (1028, False)):
        assert L.pt_model_dim_supported(dim, _native.PT_TRANSE) == int(ok)
        wide = [torch.zeros(4, 2 * dim, device=dev), torch.zeros(2, dim, device=dev)]
        d = desc(_native.PT_SGD)
        d.ent_total, d.rel_total, d.dim, d.ent, d.rel = 4, 2, dim, wide[0].data_ptr(), wide[1].data_ptr()
        if ok:
            _native.check(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)))
            L.pt_trainer_free(h)
        else:
            expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), PT_ENOTSUP, "RotatE", str(dim))
    b = [torch.zeros(50 * 3, dtype=torch.int64, device=dev) for _ in range(3)]
    # SGD trainer: no captured run, no in-kernel sampling, no timed run, no reference-order mode
    t = trainer(_native.PT_SGD)
    ms4 = (ctypes.c_float * 4)()
    expect(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), PT_ENOTSUP, "PT_ROTATE",
           "external batches")
    expect(L.pt_trainer_step(t, sampler, 50, 2, 0, 1, None, None, None, _native.ptr(losses), st), PT_ENOTSUP,
           "PT_ROTATE")
    expect(L.pt_trainer_run_timed(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), ms4, st), PT_ENOTSUP, "PT_ROTATE")
    expect(L.pt_trainer_set_deterministic(t, 1), PT_ENOTSUP, "PT_ROTATE")
    # a step without the model margin in the loss descriptor (none set, or one without score_margin_flag)
    expect(L.pt_trainer_step(t, None, 50, 2, 0, 0, _native.ptr(b[0]), _native.ptr(b[1]), _native.ptr(b[2]),
                             _native.ptr(losses), st), PT_ENOTSUP, "PT_ROTATE", "score_margin_flag")
    ld = loss_desc(_native.PT_LOSS_SIGMOID, 1, 0)
    _native.check(L.pt_trainer_set_loss(t, ctypes.byref(ld)))
    expect(L.pt_trainer_step(t, None, 50, 2, 0, 0, _native.ptr(b[0]), _native.ptr(b[1]), _native.ptr(b[2]),
                             _native.ptr(losses), st), PT_ENOTSUP, "PT_ROTATE", "score_margin_flag")
    # neg past the LDS score buffer
    ld = loss_desc(_native.PT_LOSS_SIGMOID, 1, 1)
    _native.check(L.pt_trainer_set_loss(t, ctypes.byref(ld)))
    big = 16384
    hb = [torch.zeros(2 * (big + 1), dtype=torch.int64, device=dev) for _ in range(3)]
    expect(L.pt_trainer_step(t, None, 2, big, 0, 0, _native.ptr(hb[0]), _native.ptr(hb[1]), _native.ptr(hb[2]),
                             _native.ptr(losses), st), PT_ENOTSUP, "too large")
    L.pt_trainer_free(t)
    # Adam: a refused run leaves the step count
    t = trainer(_native.PT_ADAM)
    a = _native.AdamState()
    a.ent_m, a.rel_m, a.ent_v, a.rel_v = (x.data_ptr() for x in moments)
    a.beta1, a.beta2, a.eps, a.step = 0.9, 0.999, 1e-8, 7
    _native.check(L.pt_trainer_set_adam(t, ctypes.byref(a)))
    expect(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), PT_ENOTSUP, "external batches")
    expect(L.pt_trainer_step(t, None, 50, 2, 0, 0, _native.ptr(b[0]), _native.ptr(b[1]), _native.ptr(b[2]),
                             _native.ptr(losses), st), PT_ENOTSUP, "score_margin_flag")
    assert L.pt_trainer_adam_step(t) == 7
    L.pt_trainer_free(t)
    # universes
    assert L.pt_universe_dim_supported(20, _native.PT_ROTATE) == 0
    job = (_native.UniverseJob * 1)()
    expect(L.pt_universes_train_ex(job, 1, _native.PT_ROTATE, 1, 1, _native.PT_SGD, 0, 1, 0, _native.ptr(losses), st),
           PT_ENOTSUP, "PT_ROTATE")
    expect(L.pt_universes_train(job, 1, _native.PT_ROTATE, 1, 1, _native.PT_SGD, 0, 1, _native.ptr(losses), st),
           PT_ENOTSUP, "PT_ROTATE")
    hs = ctypes.c_void_p()
    expect(L.pt_universe_set_create(job, 1, _native.PT_ROTATE, 1, 1, _native.PT_SGD, 0, 1, ctypes.byref(hs)),
           PT_ENOTSUP, "PT_ROTATE")
    us = (_native.LpUniverse * 1)()
    pairs = (_native.LpPair * 1)()
    rows = torch.full((E,), 7.0, device=dev)
    expect(L.pt_lp_min_scores(us, 1, _native.PT_ROTATE, 1, 1, pairs, 1, E, _native.ptr(rows), None, st), PT_ENOTSUP,
           "PT_ROTATE")
    torch.cuda.synchronize()
    assert (rows == 7.0).all() and not losses.any()
    for x, y in zip(tabs, keep):
        assert torch.equal(x, y)
    assert not any(m.any() for m in moments)
