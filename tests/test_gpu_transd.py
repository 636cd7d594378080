"""TransD on the GPU (k_step_transd, k_score_transd, k_score_queries_transd; transd.hip) against the float64
reference tests/transd_reference.py and the reference implementation's own runs (tests/golden/transd_*.npz).

Gradient parity runs SGD at lr 1 on explicit batches (transd_cases.py), so the table delta is the gradient:
    |delta_gpu - delta_ref64| <= tol = min(1e-5, max(4 * 2^-23 * max(1, |g|max), 4 * GRAD_DEV[family]))
for every cell of all four tables (test_gpu_adv.py's bound and reasons), and the loss to rtol 1e-5. Scores:
    |got - ref64| <= tol(D) * max(1, ref64),  tol(D) = min(1e-5, max(4 * 2^-23, 4 * SCORE_DEV[D]))
(test_gpu_lp_values.py's rule). The input conditions of the seeds are asserted on the CPU in
test_transd_reference_cpu.py. Every test prints its observed maxima.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
import transd_cases as tc
import transd_reference as tr
from conftest import KG_SMALL
from helpers import golden, load
from test_transd_reference_cpu import lp_excused

pytestmark = pytest.mark.gpu

B1, B2 = 0.9, 0.999
PT_EINVAL, PT_ENOTSUP = 1, 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible HIP device"


def _model(tabs, cfg, margin=None, epsilon=None):
    from openke.module.model import TransD
    kge = TransD(tabs[0].shape[0], tabs[1].shape[0], dim_e=cfg["dim"], dim_r=cfg["dim"], p_norm=cfg["p_norm"],
                 norm_flag=cfg["norm_flag"], margin=margin, epsilon=epsilon)
    for name, x in zip(tr.TABLES, tabs):
        getattr(kge, name).weight.data.copy_(torch.from_numpy(np.asarray(x)))
    return kge


def _trainer(tabs, cfg, opt, lr):
    """(kge, Trainer) for a TransD holding the given tables, on the GPU."""
    from openke.config import Trainer
    from openke.module.loss import MarginLoss
    from openke.module.strategy import NegativeSampling
    kge = _model(tabs, cfg)
    ns = NegativeSampling(model=kge, loss=MarginLoss(margin=cfg["loss_margin"]), batch_size=cfg["batch_size"])
    ns.cuda()
    return kge, Trainer(model=ns, data_loader=None, train_times=0, alpha=lr, use_gpu=True, opt_method=opt)


def _tables(kge):
    return [t.detach().cpu().numpy().copy() for t in kge.tables() if t is not None]


def _check_step(tag, tabs, got, grads, aux, cfg, loss, want_loss, transform=None):
    tol = tr.grad_bound(tr.family(cfg), aux["gmax"])
    for i in range(4):
        want = grads[i] if transform is None else transform(i, grads[i])
        dev = float(np.abs((np.asarray(tabs[i], dtype=np.float64) - got[i].astype(np.float64)) - want).max())
        print("%s %s: max |delta_gpu - delta_ref64| %.3e (tol %.3e, |g|max %.3e)" % (tag, tr.TABLES[i], dev, tol,
                                                                                   aux["gmax"]))
        assert dev <= tol, (tag, tr.TABLES[i], dev, tol)
    print("%s loss gpu %.9g ref %.9g" % (tag, loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)


# ------------------------------------------------------------------ 1. gradient parity ----------
@pytest.mark.parametrize("case", tc.GRAD_CASES, ids=lambda c: c[0])
def test_gradient_parity_sgd(case):
    tabs, hrt, cfg, mode = tc.build(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    flags = tc.planted(*hrt, bs, K, mode)
    assert all(v for k, v in flags.items() if k != "other_relation") and flags["other_relation"] == (mode == "normal")
    want_loss, grads, aux = tr.loss_and_grads(tabs, *hrt, bs, cfg, mode)
    kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
    loss = trn.train_one_step(tc.as_batch(hrt, bs, mode))
    got = _tables(kge)
    _check_step(case[0], tabs, got, grads, aux, cfg, loss, want_loss)
    # the entity and the relation no slot names: all four rows bit-identical
    for i, row in ((0, tc.FREE_ENT), (2, tc.FREE_ENT), (1, tc.FREE_REL), (3, tc.FREE_REL)):
        np.testing.assert_array_equal(got[i][row], tabs[i][row])


# ------------------------------------------------------------------ 2. Adagrad -------------------
def test_gradient_parity_adagrad():
    """The same step through Adagrad (k_apply, twice) from a given state_sum in [1, 2): |d delta / d g| <= 1 there,
    so the gradient bound holds for the delta; all four tables and their state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    case = tc.ADAGRAD_CASE
    tabs, hrt, cfg, mode = tc.build(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = tr.loss_and_grads(tabs, *hrt, bs, cfg, mode)
    kge, trn = _trainer(tabs, cfg, "adagrad", 1.0)
    trn.optimizer = NativeOptimizer(_native.PT_ADAGRAD, 1.0, kge.tables())
    rng = np.random.default_rng(77)
    state = [rng.uniform(1, 2, size=t.shape).astype(np.float32) for t in tabs]
    sums = [s for s in trn.optimizer.state_sum if s is not None]
    assert len(sums) == 4
    for s, x in zip(sums, state):
        s.copy_(torch.from_numpy(x))
    loss = trn.train_one_step(tc.as_batch(hrt, bs, mode))
    got = _tables(kge)
    _check_step("adagrad", tabs, got, grads, aux, cfg, loss, want_loss,
                lambda i, g: g / (np.sqrt(state[i].astype(np.float64) + g ** 2) + 1e-10))
    tol = tr.grad_bound(tr.family(cfg), aux["gmax"])
    for i, s in enumerate(sums):
        dev = float(np.abs(s.cpu().numpy().astype(np.float64) - (state[i].astype(np.float64) + grads[i] ** 2)).max())
        assert dev <= 2.0 ** -22 + 2 * aux["gmax"] * tol, (i, dev)


# ------------------------------------------------------------------ 3. Adam ----------------------
@pytest.mark.parametrize("case", tc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_three_steps_from_given_state(case):
    """After every step, for all four tables: exp_avg / exp_avg_sq within (1 - b1) tol / (1 - b2) 2 |g|max tol of the
    float64 update at the GPU's own pre-step state, every weight the float64 update formula at the GPU's own new
    moments (4 ulp of w + 1e-6 |delta|); the row touched in step 1 only keeps moving, the row never touched stays put
    with zero state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, batches, cfg, (m0, v0), lr, step0 = tc.build_adam(case)
    bs = cfg["batch_size"]
    kge, trn = _trainer(tabs, cfg, "adam", lr)
    trn.optimizer = NativeOptimizer(_native.PT_ADAM, lr, kge.tables())
    opt = trn.optimizer
    ms = [x for x in opt.exp_avg if x is not None]
    vs = [x for x in opt.exp_avg_sq if x is not None]
    assert len(ms) == 4 and len(vs) == 4
    for dst, src in zip(ms + vs, m0 + v0):
        dst.copy_(torch.from_numpy(src))
    opt.step = step0

    def state():
        return [x.detach().cpu().numpy().copy() for x in ms], [x.detach().cpu().numpy().copy() for x in vs]

    w = _tables(kge)
    m, v = state()
    once, free = tc.ONCE_ENT, tc.FREE_ENT
    for s, hrt in enumerate(batches):
        want_loss, grads, aux = tr.loss_and_grads(w, *hrt, bs, cfg)
        loss = trn.train_one_step(tc.as_batch(hrt, bs, "normal"))
        assert opt.step == step0 + s + 1
        assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
        w2 = _tables(kge)
        m2, v2 = state()
        tol = tr.grad_bound(tr.family(cfg), aux["gmax"])
        for i in range(4):
            _, mr, vr = tr.adam_update(w[i], m[i], v[i], grads[i], lr, opt.step)
            dm, dv = float(np.abs(m2[i] - mr).max()), float(np.abs(v2[i] - vr).max())
            print("%s step %d %s: |m - ref| %.3e (bound %.3e), |v - ref| %.3e (bound %.3e)"
                  % (case[0], s, tr.TABLES[i], dm, (1 - B1) * tol, dv, (1 - B2) * 2 * aux["gmax"] * tol))
            assert dm <= (1 - B1) * tol
            assert dv <= (1 - B2) * 2 * aux["gmax"] * tol
            wr = tr.adam_weights(w[i], m2[i], v2[i], lr, opt.step)
            bound = 4 * np.spacing(np.abs(w[i])).astype(np.float64) + 1e-6 * np.abs(wr - w[i])
            assert (np.abs(w2[i].astype(np.float64) - wr) <= bound).all(), (case[0], s, i)
        for i in (0, 2):   # entity 35: touched in step 1 only, still moving; entity 36: never touched
            assert (w2[i][once] != w[i][once]).any(), "row %d must move in step %d" % (once, s + 1)
            assert (grads[i][once] != 0).any() == (s == 0)
            assert (w2[i][free] == tabs[i][free]).all() and not m2[i][free].any() and not v2[i][free].any()
        w, m, v = w2, m2, v2


@pytest.mark.parametrize("path", golden("transd_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_optimizer_runs_match_reference_trajectories(path):
    """The reference implementation's 10-step Adam and Adagrad runs: losses to rtol 1e-4, every table element within
    the caps of test_optimizer_runs_match_reference (Adam's per-step bound for two trajectories; Adagrad steps * lr *
    1e-3). A sanity cap: the parity proof is the tests above."""
    z = load(path)
    cfg = tr.golden_cfg(z)
    lr, steps, opt = float(z["lr"]), int(z["steps"]), str(z["optimizer"])
    kge, trn = _trainer([np.array(x) for x in tr.golden_tables(z, "init")], cfg, opt, lr)
    for s in range(steps):
        batch = {"batch_h": z["b%d_h" % s], "batch_t": z["b%d_t" % s], "batch_r": z["b%d_r" % s],
                 "mode": str(z["modes"][s])}
        loss = trn.train_one_step(batch)
        assert abs(loss - float(z["losses"][s])) <= 1e-4 * abs(float(z["losses"][s])), (s, loss, float(z["losses"][s]))
    if opt == "adam":
        assert trn.optimizer.step == steps
    cap = 2 * steps * lr * (1 - B1) / np.sqrt(1 - B2) if opt == "adam" else steps * lr * 1e-3
    for got, want, name in zip(_tables(kge), tr.golden_tables(z, "final"), tr.TABLES):
        dev = float(np.abs(got - want).max())
        print("%s %s: |final - ref| %.3e (cap %.3e)" % (path.split("/")[-1], name, dev, cap))
        assert dev <= cap


# ------------------------------------------------------------------ 4. reference steps ----------
@pytest.mark.parametrize("path", golden("transd_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_reference_steps_teacher_forced(path):
    """Every recorded step of the reference implementation, from its own tables before the step: the GPU delta within
    the parity bound of the float64 gradient, the loss to rtol 1e-5 of float64 (and so of the recorded one)."""
    z = load(path)
    cfg = tr.golden_cfg(z)
    bs = cfg["batch_size"]
    for s in range(int(z["steps"])):
        tabs = [np.array(x) for x in tr.golden_tables(z, "s%d" % s)]
        (h, t, r), mode = tr.golden_step(z, cfg, s)
        want_loss, grads, aux = tr.loss_and_grads(tabs, h, t, r, bs, cfg, mode)
        kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
        batch = {"batch_h": z["b%d_h" % s], "batch_t": z["b%d_t" % s], "batch_r": z["b%d_r" % s], "mode": mode}
        loss = trn.train_one_step(batch)
        _check_step("%s step %d" % (path.split("/")[-1], s), tabs, _tables(kge), grads, aux, cfg, loss, want_loss)
        assert abs(loss - float(z["losses"][s])) <= 1e-5 * abs(float(z["losses"][s]))


# ------------------------------------------------------------------ 5. scores --------------------
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


@pytest.mark.parametrize("D", tr.SCORE_DIMS)
def test_scores_match_float64(D):
    """pt_score in the three modes (through predict), pt_score_queries and pt_score_rows on both sides."""
    from openke import _native
    L = _native.lib()
    tol = tr.score_tol(D)
    worst = 0.0
    for p in (1, 2):
        for nf in (True, False):
            tabs, batches, cfg = tr.score_case(D, p, nf)
            kge = _model(tabs, cfg).cuda()
            for mode, (h, t, r) in batches.items():
                got = kge.predict({"batch_h": h, "batch_t": t, "batch_r": r, "mode": mode}).astype(np.float64)
                ref = tr.scores(tabs, *tr.expand_predict(h, t, r, mode), cfg, mode)
                err = np.abs(got - ref) / np.maximum(1.0, ref)
                worst = max(worst, float(err.max()))
                assert (err <= tol).all(), (D, p, nf, mode, float(err.max()), tol)
            h, t, r = batches["normal"]
            nq = 5
            for side in (0, 1):
                ref = np.stack([tr.lp_scores(tabs, int(t[i] if side == 0 else h[i]), int(r[i]), side, cfg)
                                for i in range(nq)])
                rows = _rows(kge, L.pt_score_rows, side, h[:nq], t[:nq], r[:nq])
                err = np.abs(rows - ref) / np.maximum(1.0, ref)
                worst = max(worst, float(err.max()))
                assert (err <= tol).all(), (D, p, nf, side, "rows", float(err.max()), tol)
                cand = _rows(kge, L.pt_score_queries, side, h[:nq], t[:nq], r[:nq])
                for i in range(nq):   # candidate order [truth, 0..E-1 without truth]
                    truth = int(h[i] if side == 0 else t[i])
                    order = oracle.candidates(tr.E, truth)
                    np.testing.assert_array_equal(cand[i], rows[i][order])
    print("D %d: worst |gpu - ref64| / max(1, ref64) %.3e (tol %.3e)" % (D, worst, tol))


def test_predict_on_a_model_with_a_margin_returns_the_distance():
    z = load(golden("transd_p2.npz")[0])
    cfg = {"p_norm": int(z["p_norm"]), "norm_flag": bool(z["norm_flag"]), "dim": int(z["dim"])}
    kge = _model(tr.golden_tables(z, ""), cfg, margin=float(z["model_margin"]), epsilon=float(z["epsilon"])).cuda()
    assert kge.margin_flag
    for mode in ("normal", "head_batch", "tail_batch"):
        got = kge.predict({"batch_h": z[mode + "_h"], "batch_t": z[mode + "_t"], "batch_r": z[mode + "_r"],
                           "mode": mode})
        want = z[mode + "_score"]
        assert (np.abs(got - want) <= 1e-5 * np.maximum(1.0, want)).all()
    fwd = kge.forward({"batch_h": z["normal_h"], "batch_t": z["normal_t"], "batch_r": z["normal_r"],
                       "mode": "normal"}).cpu().numpy()
    np.testing.assert_allclose(fwd, float(z["model_margin"]) - z["normal_score"], rtol=0, atol=1e-5)


# ------------------------------------------------------------------ 6. link prediction ----------
def test_link_prediction_matches_reference_ranks():
    """Tester.run_link_prediction on kg_small with the recorded tables: every query's raw and filtered rank equal to
    the reference's unless its float64 score vector holds a candidate within 4e-6 relative of the truth; metrics
    equal when no query is excused."""
    from openke.config import Tester
    from openke.data import TestDataLoader
    z = load(golden("transd_lp.npz")[0])
    cfg = {"p_norm": int(z["p_norm"]), "norm_flag": bool(z["norm_flag"]), "dim": int(z["dim"])}
    tabs = tr.golden_tables(z, "")
    test_dl = TestDataLoader(KG_SMALL, "link")
    tester = Tester(model=_model(tabs, cfg), data_loader=test_dl, use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    q = z["queries"].astype(np.int64)
    h, t, r = test_dl.eval_triples()
    np.testing.assert_array_equal(np.stack([h, t, r], 1), q)
    excused = lp_excused(tabs, q, cfg)
    assert excused.any(axis=0).mean() <= 0.02
    want = z["ranks"].astype(np.int64)
    differ = 0
    for k, g in enumerate(tester.last_ranks):
        d = np.asarray(g, dtype=np.int64) != want[k]
        assert not (d & ~excused[k // 2]).any(), (str(z["rank_names"][k]), np.nonzero(d & ~excused[k // 2])[0][:10])
        differ += int(d.sum())
    print("transd_lp: %d ranks differ, %d (query, side) pairs excused" % (differ, int(excused.sum())))
    if not excused.any():
        assert differ == 0
        np.testing.assert_array_equal(np.array(res, dtype=np.float32), z["metrics"].astype(np.float32))


# ------------------------------------------------------------------ 7. example-shaped run -------
def test_example_shaped_run_link_prediction_and_checkpoint(tmp_path):
    """Trainer.run() in the shape of examples/train_transd_FB15K237.py on kg_small, then Tester.run_link_prediction,
    then save_checkpoint -> a fresh TransD -> load_checkpoint."""
    from openke.config import Tester, Trainer
    from openke.data import TestDataLoader, TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransD
    from openke.module.strategy import NegativeSampling
    threads, bs, neg, seed, epochs = 8, 150, 8, 33, 3
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=bs, threads=threads, sampling_mode="normal", bern_flag=1,
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
    nb = dl.nbatches
    torch.manual_seed(6)
    kge = TransD(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim_e=32, dim_r=32, p_norm=1, norm_flag=True)
    ns = NegativeSampling(model=kge, loss=MarginLoss(margin=4.0), batch_size=dl.get_batch_size())
    trn = Trainer(model=ns, data_loader=dl, train_times=epochs, alpha=1.0, use_gpu=True)
    trn.run()
    assert len(trn.epoch_losses) == epochs and np.isfinite(trn.epoch_losses).all()
    assert np.isfinite(trn.last_step_losses).all()
    assert trn.epoch_losses[-1] < trn.epoch_losses[0]
    # the sampler streams advanced by exactly epochs * nbatches loader calls
    kg = oracle.KG.load(KG_SMALL)
    st = oracle.GlibcRand(seed).rand_reset(threads)
    for _ in range(epochs * nb + 1):
        h, t, r, _y = kg.sample_ex(st, threads, bs, neg, 0, 0, 1, 1)
    dl.sampling()
    np.testing.assert_array_equal(dl.batch_h, h)
    np.testing.assert_array_equal(dl.batch_t, t)
    np.testing.assert_array_equal(dl.batch_r, r)
    tester = Tester(model=kge, data_loader=TestDataLoader(KG_SMALL, "link"), use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    assert np.isfinite(np.asarray(res, dtype=np.float64)).all()
    data = {"batch_h": h[:64], "batch_t": t[:64], "batch_r": r[:64], "mode": "normal"}
    before = kge.predict(data)
    path = os.path.join(str(tmp_path), "transd.ckpt")
    kge.save_checkpoint(path)
    torch.manual_seed(99)
    fresh = TransD(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim_e=32, dim_r=32, p_norm=1,
                   norm_flag=True).cuda()
    assert not np.array_equal(fresh.predict(data), before)
    fresh.load_checkpoint(path)
    np.testing.assert_array_equal(fresh.predict(data), before)


# ------------------------------------------------------------------ 8. refusals -----------------
def _small(**kw):
    from openke.module.model import TransD
    torch.manual_seed(1)
    return TransD(6, 2, dim_e=8, dim_r=8, **kw)


def _ns(kge, loss, **kw):
    from openke.module.strategy import NegativeSampling
    return NegativeSampling(model=kge, loss=loss, batch_size=2, **kw)


BATCH = {"batch_h": np.array([0, 1, 2, 3]), "batch_t": np.array([1, 2, 3, 4]), "batch_r": np.array([0, 1, 0, 1]),
         "mode": "normal"}


def test_unsupported_python_combinations_raise():
    from openke.config import Parallel_Universe_Config, Trainer
    from openke.module.loss import MarginLoss, SigmoidLoss
    from openke.module.model import TransD
    with pytest.raises(NotImplementedError, match="dim_e != dim_r"):
        TransD(6, 2, dim_e=8, dim_r=12)
    cases = [
        (_ns(_small(), SigmoidLoss()), {}, "TransE only"),
        (_ns(_small(), MarginLoss(adv_temperature=1.0)), {}, "TransE only"),
        (_ns(_small(margin=3.0), MarginLoss()), {}, "TransE only"),
        (_ns(_small(), MarginLoss()), {"deterministic": True}, "not implemented for TransD"),
    ]
    for ns, kw, frag in cases:
        kge = ns.model
        w0 = [t.detach().clone() for t in kge.tables() if t is not None]
        trn = Trainer(model=ns, data_loader=None, train_times=0, alpha=0.1, use_gpu=True, **kw)
        with pytest.raises(NotImplementedError, match=frag):
            trn.train_one_step(BATCH)
        for a, b in zip(w0, [t for t in kge.tables() if t is not None]):
            assert torch.equal(a, b.detach().cpu())
    pu = object.__new__(Parallel_Universe_Config)
    pu.embedding_model = TransD
    with pytest.raises(NotImplementedError, match="PuTransD is not built yet"):
        pu._check_setup()


def test_unsupported_native_combinations_are_refused():
    """pt_trainer_run, in-kernel sampling, pt_trainer_run_timed, the reference-order mode, a non-default loss and the
    universe entry points with PT_TRANSD: PT_ENOTSUP / PT_EINVAL with a message, rows untouched, the Adam step count
    unchanged."""
    from openke import _native
    from openke.data import TrainDataLoader
    L = _native.lib()
    dev = torch.device("cuda", 0)
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=50, threads=8, bern_flag=0, filter_flag=1, neg_ent=2,
                         random_seed=3)
    sampler = dl.device_sampler()
    E, R, D = dl.get_ent_tot(), dl.get_rel_tot(), 8
    mk = lambda rows: torch.rand(rows, D, device=dev) - 0.5
    tabs = [mk(E), mk(R), mk(E), mk(R)]
    keep = [x.clone() for x in tabs]
    moments = [torch.zeros_like(x) for x in tabs + tabs]
    losses = torch.zeros(4, device=dev)
    st = _native.stream()

    def desc(opt, transfer=True):
        d = _native.ModelDesc()
        d.model, d.p_norm, d.norm_flag, d.opt, d.lr, d.margin = _native.PT_TRANSD, 1, 1, opt, 0.1, 2.0
        d.ent_total, d.rel_total, d.dim = E, R, D
        d.ent, d.rel = tabs[0].data_ptr(), tabs[1].data_ptr()
        if transfer:
            d.ent_transfer, d.rel_transfer = tabs[2].data_ptr(), tabs[3].data_ptr()
        return d

    def trainer(opt):
        h = ctypes.c_void_p()
        d = desc(opt)
        _native.check(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)))
        return h

    def expect(rc, code, *words):
        assert rc == code, (rc, L.pt_last_error().decode())
        msg = L.pt_last_error().decode()
        assert all(w in msg for w in words), msg

    # the descriptor: both transfer tables, and their Adagrad state under PT_ADAGRAD
    h = ctypes.c_void_p()
    d = desc(_native.PT_SGD, transfer=False)
    expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), PT_EINVAL, "ent_transfer")
    d = desc(_native.PT_ADAGRAD)
    d.ent_acc, d.rel_acc = moments[0].data_ptr(), moments[1].data_ptr()
    expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), PT_EINVAL, "state_sum")
    # SGD trainer: no captured run, no in-kernel sampling, no timed run, no reference-order mode, no other loss
    t = trainer(_native.PT_SGD)
    ms4 = (ctypes.c_float * 4)()
    expect(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), PT_ENOTSUP, "PT_TRANSD",
           "external batches")
    expect(L.pt_trainer_step(t, sampler, 50, 2, 0, 1, None, None, None, _native.ptr(losses), st), PT_ENOTSUP,
           "PT_TRANSD")
    expect(L.pt_trainer_run_timed(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), ms4, st), PT_ENOTSUP, "PT_TRANSD")
    expect(L.pt_trainer_set_deterministic(t, 1), PT_ENOTSUP, "TransD")
    for kind, adv, flag in ((_native.PT_LOSS_SIGMOID, 0, 0), (_native.PT_LOSS_MARGIN, 1, 0),
                            (_native.PT_LOSS_MARGIN, 0, 1)):
        ld = _native.LossDesc()
        ld.kind, ld.adv, ld.temperature, ld.score_margin_flag, ld.score_margin = kind, adv, 1.0, flag, 3.0
        expect(L.pt_trainer_set_loss(t, ctypes.byref(ld)), PT_ENOTSUP, "TransE only")
    L.pt_trainer_free(t)
    # Adam: the moments of all four tables; a refused run leaves the step count
    t = trainer(_native.PT_ADAM)
    a = _native.AdamState()
    a.ent_m, a.rel_m, a.ent_v, a.rel_v = (x.data_ptr() for x in (moments[0], moments[1], moments[4], moments[5]))
    a.beta1, a.beta2, a.eps, a.step = 0.9, 0.999, 1e-8, 7
    expect(L.pt_trainer_set_adam(t, ctypes.byref(a)), PT_EINVAL, "every table")
    a.ent_transfer_m, a.rel_transfer_m = moments[2].data_ptr(), moments[3].data_ptr()
    a.ent_transfer_v, a.rel_transfer_v = moments[6].data_ptr(), moments[7].data_ptr()
    _native.check(L.pt_trainer_set_adam(t, ctypes.byref(a)))
    expect(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), PT_ENOTSUP, "external batches")
    assert L.pt_trainer_adam_step(t) == 7
    L.pt_trainer_free(t)
    # universes
    assert L.pt_universe_dim_supported(20, _native.PT_TRANSD) == 0
    job = (_native.UniverseJob * 1)()
    expect(L.pt_universes_train_ex(job, 1, _native.PT_TRANSD, 1, 1, _native.PT_SGD, 0, 1, 0, _native.ptr(losses), st),
           PT_ENOTSUP, "PuTransD")
    us = (_native.LpUniverse * 1)()
    pairs = (_native.LpPair * 1)()
    rows = torch.full((E,), 7.0, device=dev)
    expect(L.pt_lp_min_scores(us, 1, _native.PT_TRANSD, 1, 1, pairs, 1, E, _native.ptr(rows), None, st), PT_ENOTSUP,
           "PuTransD")
    torch.cuda.synchronize()
    assert (rows == 7.0).all() and not losses.any()
    for x, y in zip(tabs, keep):
        assert torch.equal(x, y)
    assert not any(m.any() for m in moments)
