"""TransE and TransH single models at dims 516..1024 (float4 rows with three and four chunks per lane) on the GPU:
scores, the plain and the weighted external-batch step, Adam, Trainer.run on both of its paths, the reference-order
mode, link prediction, the example's configuration and the refusals, against the float64 references
(adv_reference.py, lp_reference.py) and the CPU oracle.

Tolerances are wide_cases.py's: the project's rules with the deviation tables measured on the CPU at these dims
(test_wide_reference_cpu.py, which also asserts the input conditions of every case here). Every test prints its
observed maxima."""
import ctypes
import os

import numpy as np
import pytest
import torch

import adv_reference as ar
import oracle
import wide_cases as wc
from conftest import KG_SMALL
from helpers import assert_step_close, metrics_match_ranks, step_noise
from lp_reference import lp_scores64
from test_oracle import call_modes

pytestmark = pytest.mark.gpu

B1, B2 = 0.9, 0.999
PT_ENOTSUP = 6
RULE = "multiples of 4 from 516 to 1024"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible HIP device"


def _model(tabs, cfg):
    from openke.module.model import TransE, TransH
    E, R = tabs[0].shape[0], tabs[1].shape[0]
    if cfg["model"] == "TransH":
        kge = TransH(E, R, dim=cfg["dim"], p_norm=cfg["p_norm"], norm_flag=cfg["norm_flag"])
        kge.norm_vector.weight.data.copy_(torch.from_numpy(tabs[2]))
    else:
        kge = TransE(E, R, dim=cfg["dim"], p_norm=cfg["p_norm"], norm_flag=cfg["norm_flag"],
                     margin=cfg.get("model_margin"))
    kge.ent_embeddings.weight.data.copy_(torch.from_numpy(tabs[0]))
    kge.rel_embeddings.weight.data.copy_(torch.from_numpy(tabs[1]))
    return kge


def _trainer(tabs, cfg, opt, lr):
    """(kge, Trainer) for a model holding the given tables, on the GPU."""
    from openke.config import Trainer
    from openke.module.loss import MarginLoss, SigmoidLoss
    from openke.module.strategy import NegativeSampling
    kge = _model(tabs, cfg)
    if cfg["loss"] == "sigmoid":
        loss = SigmoidLoss(adv_temperature=cfg["adv_temperature"])
    else:
        loss = MarginLoss(adv_temperature=cfg["adv_temperature"], margin=cfg["loss_margin"])
    ns = NegativeSampling(model=kge, loss=loss, batch_size=cfg["batch_size"])
    ns.cuda()
    return kge, Trainer(model=ns, data_loader=None, train_times=0, alpha=lr, use_gpu=True, opt_method=opt)


def _tables(kge):
    return [t.detach().cpu().numpy().copy() for t in kge.tables() if t is not None]


def _check_delta(tag, tabs, got, want, tol, gmax):
    for i, w in enumerate(want):
        dev = float(np.abs((tabs[i].astype(np.float64) - got[i].astype(np.float64)) - w).max())
        print("%s table %d: max |delta_gpu - delta_ref64| %.3e (tol %.3e, |g|max %.3e)" % (tag, i, dev, tol, gmax))
        assert dev <= tol, (tag, i, dev, tol)


# ------------------------------------------------------------------ 1. scores --------------------
def _rows(kge, side, qh, qt, qr):
    from openke import _native
    dev = kge.ent_embeddings.weight.device
    E = kge.ent_embeddings.weight.shape[0]
    q = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(dev) for x in (qh, qt, qr)]
    out = torch.full((len(qh), E), -1.0, dtype=torch.float32, device=dev)
    desc = kge.native_desc()
    _native.check(_native.lib().pt_score_rows(ctypes.byref(desc), side, _native.ptr(q[0]), _native.ptr(q[1]),
                                              _native.ptr(q[2]), len(qh), _native.ptr(out), _native.stream()))
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("model", ["TransE", "TransH"])
@pytest.mark.parametrize("D", wc.WIDE_DIMS)
def test_scores_match_float64(D, model):
    """predict in its three modes (k_score) and pt_score_rows on both sides (k_score_queries), p 1 / 2 with and without
    normalisation: every cell within tol(D) of the float64 reference."""
    tol = wc.score_tol(D)
    worst = 0.0
    for p in (1, 2):
        for nf in (True, False):
            tabs, batches = wc.score_case(model, D, p, nf)
            kge = _model(tabs, {"model": model, "dim": D, "p_norm": p, "norm_flag": nf}).cuda()
            for mode, (h, t, r) in batches.items():
                got = kge.predict({"batch_h": h, "batch_t": t, "batch_r": r, "mode": mode}).astype(np.float64)
                ref = wc.scores64(model, p, nf, tabs, *wc.expand_predict(h, t, r))
                err = np.abs(got - ref) / np.maximum(1.0, ref)
                worst = max(worst, float(err.max()))
                assert (err <= tol).all(), (D, model, p, nf, mode, float(err.max()), tol)
            h, t, r = batches["normal"]
            nq = 5
            for side in (0, 1):
                ref = np.stack([lp_scores64(model, p, nf, tabs[0], tabs[1], tabs[2], int(t[i] if side == 0 else h[i]),
                                            int(r[i]), side) for i in range(nq)])
                rows = _rows(kge, side, h[:nq], t[:nq], r[:nq])
                err = np.abs(rows - ref) / np.maximum(1.0, ref)
                worst = max(worst, float(err.max()))
                assert (err <= tol).all(), (D, model, p, nf, side, "rows", float(err.max()), tol)
    print("%s D %d: worst |gpu - ref64| / max(1, ref64) %.3e (tol %.3e)" % (model, D, worst, tol))


# ------------------------------------------------------------------ 2. the plain step -----------
@pytest.mark.parametrize("case", wc.PLAIN_CASES, ids=lambda c: c[0])
def test_plain_step_gradient_parity(case):
    """k_step + k_apply on an external batch under SGD lr 1 (the table delta is the gradient) or Adagrad lr 1 from a
    given state_sum in [1, 2) (|d delta / d g| <= 1 there): every cell of every table within the gradient bound, the
    loss to rtol 1e-5, the rows no slot names bit-identical."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, hrt, cfg = wc.build_plain(case)
    tabs = [x for x in tabs if x is not None]
    bs, opt = cfg["batch_size"], case[7]
    want_loss, grads, aux = ar.loss_and_grads(tabs, *hrt, bs, cfg)
    kge, tr = _trainer(tabs + [None], cfg, opt, 1.0)
    want = grads
    if opt == "adagrad":
        tr.optimizer = NativeOptimizer(_native.PT_ADAGRAD, 1.0, kge.tables())
        rng = np.random.default_rng(77)
        state = [rng.uniform(1, 2, size=t.shape).astype(np.float32) for t in tabs]
        for s, x in zip([s for s in tr.optimizer.state_sum if s is not None], state):
            s.copy_(torch.from_numpy(x))
        want = [g / (np.sqrt(state[i].astype(np.float64) + g ** 2) + 1e-10) for i, g in enumerate(grads)]
    loss = tr.train_one_step(wc.as_batch(hrt))
    got = _tables(kge)
    _check_delta(case[0], tabs, got, want, wc.grad_tol(aux["gmax"], cfg), aux["gmax"])
    print("%s loss gpu %.9g ref %.9g" % (case[0], loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
    np.testing.assert_array_equal(got[0][wc.FREE_ENT], tabs[0][wc.FREE_ENT])
    for i in range(1, len(tabs)):
        np.testing.assert_array_equal(got[i][wc.FREE_REL], tabs[i][wc.FREE_REL])


# ------------------------------------------------------------------ 3. the weighted step --------
@pytest.mark.parametrize("case", wc.ADV_CASES + wc.STABILITY_CASES, ids=lambda c: c[0])
def test_weighted_step_gradient_parity(case):
    """k_step_adv (TransE): the four loss families and the temperature-40 stability case at every wide dim, K = 3, 7
    and 70, under SGD lr 1: finite, every cell of both tables within the gradient bound, the loss to rtol 1e-5."""
    tabs, batch, cfg = wc.build_adv(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = ar.loss_and_grads(tabs, *wc.expanded(batch, bs), bs, cfg)
    kge, tr = _trainer(tabs, cfg, "sgd", 1.0)
    loss = tr.train_one_step(batch)
    got = _tables(kge)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in got)
    _check_delta(case[0], tabs, got, grads, wc.grad_tol(aux["gmax"], cfg), aux["gmax"])
    print("%s loss gpu %.9g ref %.9g" % (case[0], loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)


# ------------------------------------------------------------------ 4. Adam ----------------------
@pytest.mark.parametrize("case", wc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_three_steps_from_given_state(case):
    """k_apply_adam after k_step_adv (TransE) and k_step (TransH), test_gpu_adv.py's bounds: after every step exp_avg /
    exp_avg_sq within (1 - b1) tol / (1 - b2) 2 |g|max tol of the float64 update at the GPU's own pre-step state,
    every weight the float64 update formula at the GPU's own new moments (4 ulp of w + 1e-6 |delta|); the row touched
    in step 1 only keeps moving, the row never touched stays put with zero state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, batches, cfg, (m0, v0), lr, step0 = wc.build_adam(case)
    bs = cfg["batch_size"]
    kge, tr = _trainer(tabs, cfg, "adam", lr)
    tr.optimizer = NativeOptimizer(_native.PT_ADAM, lr, kge.tables())
    opt = tr.optimizer
    for dst, src in zip(opt.exp_avg + opt.exp_avg_sq, m0 + v0):
        if src is not None:
            dst.copy_(torch.from_numpy(src))
    opt.step = step0
    ms = [x for x in opt.exp_avg if x is not None]
    vs = [x for x in opt.exp_avg_sq if x is not None]

    def state():
        return [x.detach().cpu().numpy().copy() for x in ms], [x.detach().cpu().numpy().copy() for x in vs]

    w0 = _tables(kge)
    w = w0
    m, v = state()
    once, free = wc.ONCE_ENT, wc.FREE_ENT
    for s, batch in enumerate(batches):
        want_loss, grads, aux = ar.loss_and_grads(w, *wc.expanded(batch, bs), bs, cfg)
        loss = tr.train_one_step(batch)
        assert opt.step == step0 + s + 1
        assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
        w2 = _tables(kge)
        m2, v2 = state()
        tol = wc.grad_tol(aux["gmax"], cfg)
        for i in range(len(w)):
            _, mr, vr = ar.adam_update(w[i], m[i], v[i], grads[i], lr, opt.step)
            dm, dv = float(np.abs(m2[i] - mr).max()), float(np.abs(v2[i] - vr).max())
            print("%s step %d table %d: |m - ref| %.3e (bound %.3e), |v - ref| %.3e (bound %.3e)"
                  % (case[0], s, i, dm, (1 - B1) * tol, dv, (1 - B2) * 2 * aux["gmax"] * tol))
            assert dm <= (1 - B1) * tol
            assert dv <= (1 - B2) * 2 * aux["gmax"] * tol
            wr = ar.adam_weights(w[i], m2[i], v2[i], lr, opt.step)
            bound = 4 * np.spacing(np.abs(w[i])).astype(np.float64) + 1e-6 * np.abs(wr - w[i])
            assert (np.abs(w2[i].astype(np.float64) - wr) <= bound).all(), (case[0], s, i)
        assert (w2[0][once] != w[0][once]).any(), "row %d must move in step %d" % (once, s + 1)
        assert (grads[0][once] != 0).any() == (s == 0)
        assert (w2[0][free] == w0[0][free]).all() and not m2[0][free].any() and not v2[0][free].any()
        w, m, v = w2, m2, v2


# ------------------------------------------------------------------ 5. Trainer.run ---------------
# p = 2 throughout: the oracle flags a slot as a near tie when some |v_i| lies within 2 (d + 8) eps of its terms'
# magnitudes, a band that grows with d over d components, so at these dims most p = 1 slots hold one and
# assert_step_close's cap on near-tie rows (2 %) cannot be met by any batch. The p = 1 gradients are held to the float64
# reference cell by cell in the plain-step and weighted-step tests above.
RUN_CASES = [
    # model, dim, p, norm_flag, opt, bs, neg, bern, filter, fused
    ("TransE", 516, 2, True, "adagrad", 40, 6, 1, 1, True),     # k_step_csr, one lane group per positive
    ("TransE", 1024, 2, False, "sgd", 24, 12, 1, 1, True),      # two lane groups per positive, raw rows
    ("TransE", 1024, 2, True, "adagrad", 16, 25, 0, 1, True),   # four lane groups per positive
    ("TransE", 516, 2, True, "sgd", 32, 2, 1, 1, False),        # neg < 4: no counting sort, so external batches
    ("TransH", 516, 2, True, "adagrad", 32, 5, 1, 1, False),
    ("TransH", 1024, 2, False, "sgd", 24, 3, 1, 0, False),
]


@pytest.mark.parametrize("case", RUN_CASES, ids=lambda c: "%s-d%d-p%d-nf%d-%s-bs%d-neg%d" % c[:7])
def test_trainer_run_steps_teacher_forced(case):
    """Trainer.run on kg_small, one step per run, three steps: wide TransE with neg >= 4 takes the fused run
    (in-kernel sampling, k_step_csr + k_apply_buf), everything else the external-batch loop, and the library's query
    says which. Every step starts from the oracle's state (tables, Adagrad state, sampler streams) and must equal the
    oracle's step as test_gpu_parity.py's teacher-forced cases do (helpers.kappa_bound); the streams end where the
    oracle's do."""
    from openke import _native
    from openke.config import Trainer
    from openke.config.Trainer import NativeOptimizer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransE, TransH
    from openke.module.strategy import NegativeSampling
    model, dim, p, nf, opt, bs, neg, bern, filt, fused = case
    lr, margin, seed, steps = (0.5 if opt == "sgd" else 0.05), 3.0, 23, 3
    L = _native.lib()
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=bs, threads=8, sampling_mode="normal", bern_flag=bern,
                         filter_flag=filt, neg_ent=neg, neg_rel=0, random_seed=seed)
    dl.nbatches = 1
    kg = oracle.KG.load(KG_SMALL)
    torch.manual_seed(dim + neg)
    kge = (TransE if model == "TransE" else TransH)(dl.get_ent_tot(), dl.get_rel_tot(), dim=dim, p_norm=p, norm_flag=nf)
    ns = NegativeSampling(model=kge, loss=MarginLoss(margin=margin), batch_size=bs)
    ns.cuda()
    tr = Trainer(model=ns, data_loader=dl, train_times=1, alpha=lr, use_gpu=True, opt_method=opt)
    ada = opt == "adagrad"
    tr.optimizer = NativeOptimizer(_native.PT_ADAGRAD if ada else _native.PT_SGD, lr, kge.tables())
    devt = list(kge.tables())
    dacc = list(tr.optimizer.state_sum)
    ent, rel, nv = (None if t is None else t.detach().cpu().numpy().copy() for t in devt)
    accs = [np.zeros_like(ent), np.zeros_like(rel), None if nv is None else np.zeros_like(nv)] if ada else [None] * 3
    st = oracle.GlibcRand(seed).rand_reset(8)
    sampler = dl.device_sampler()
    for k in range(steps):
        with torch.no_grad():
            for d_, h_ in zip(devt + dacc, [ent, rel, nv] + accs):
                if h_ is not None:
                    d_.copy_(torch.from_numpy(h_))
        _native.check(L.pt_sampler_set_seeds(sampler, st.ctypes.data))
        tr.run()
        assert tr.last_run_fused == fused
        assert L.pt_trainer_fused_supported(tr._native, bs, neg) == int(fused)
        loss = float(tr.last_step_losses[0])
        got = [None if t is None else t.detach().cpu().numpy() for t in devt]
        got_acc = [None if t is None else t.cpu().numpy() for t in dacc]
        acc0 = [None if a is None else a.copy() for a in accs]
        tab0 = [None if a is None else a.copy() for a in (ent, rel, nv)]
        h, t, r, _ = kg.sample(st, 8, bs, neg, bern, filt)
        gm = oracle.grad_mass(model, p, nf, margin, ent, rel, nv, h, t, r, bs, neg)
        want = oracle.train_step(model, p, nf, opt, lr, margin, ent, rel, nv, accs, h, t, r, bs, neg)
        assert abs(loss - want) <= 1e-5 * max(1.0, abs(want)), (k, loss, want)
        for i, name in enumerate(("ent", "rel", "norm")):
            w = (ent, rel, nv)[i]
            if w is None:
                continue
            mask = step_noise(acc0[i], accs[i], got_acc[i]) if ada else None
            ratio = assert_step_close(got[i], w, 2e-6, mask, what="step %d %s" % (k, name), before=tab0[i],
                                      gm=gm[name], lr=lr, acc_before=acc0[i])
            print("step %d %s: worst error / rounding bound %.3f" % (k, name, ratio))
    nxt = np.zeros(8, dtype=np.uint64)
    _native.check(L.pt_sampler_get_seeds(sampler, nxt.ctypes.data))
    np.testing.assert_array_equal(nxt, st)


# ------------------------------------------------------------------ 6. reference-order mode ------
@pytest.mark.parametrize("model,p,neg", [("TransE", 1, 3), ("TransH", 2, 2)])
def test_deterministic_trainer_run_bit_exact(model, p, neg):
    """Trainer(deterministic=True).run() at dim 516 with Adagrad, three steps: tables, state_sum and every step's loss
    equal to the oracle's, bit for bit."""
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransE, TransH
    from openke.module.strategy import NegativeSampling
    dim, nf, bs, bern, filt, steps, lr, margin, seed = 516, True, 40, 1, 1, 3, 0.05, 3.0, 17
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=bs, threads=8, sampling_mode="normal", bern_flag=bern,
                         filter_flag=filt, neg_ent=neg, neg_rel=0, random_seed=seed)
    dl.nbatches = steps
    torch.manual_seed(dim + neg)
    kge = (TransE if model == "TransE" else TransH)(dl.get_ent_tot(), dl.get_rel_tot(), dim=dim, p_norm=p, norm_flag=nf)
    ent, rel = (x.detach().numpy().copy() for x in kge.tables()[:2])
    nv = kge.tables()[2].detach().numpy().copy() if model == "TransH" else None
    ns = NegativeSampling(model=kge, loss=MarginLoss(margin=margin), batch_size=bs)
    tr = Trainer(model=ns, data_loader=dl, train_times=1, alpha=lr, use_gpu=True, opt_method="adagrad",
                 deterministic=True)
    tr.run()
    assert tr.last_run_fused   # (the reference-order run is dim-generic: no external-batch loop)
    kg = oracle.KG.load(KG_SMALL)
    st = oracle.GlibcRand(seed).rand_reset(8)
    accs = (np.zeros_like(ent), np.zeros_like(rel), None if nv is None else np.zeros_like(nv))
    losses = []
    for _ in range(steps):
        h, t, r, _ = kg.sample(st, 8, bs, neg, bern, filt)
        losses.append(oracle.train_step(model, p, nf, "adagrad", lr, margin, ent, rel, nv, accs, h, t, r, bs, neg))
    np.testing.assert_array_equal(tr.last_step_losses, np.array(losses, dtype=np.float32))
    for got, want in zip(_tables(kge), [x for x in (ent, rel, nv) if x is not None]):
        np.testing.assert_array_equal(got, want)
    for got, want in zip([a for a in tr.optimizer.state_sum if a is not None], [a for a in accs if a is not None]):
        np.testing.assert_array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------ 7. link prediction ----------
@pytest.mark.parametrize("case", wc.LP_CASES, ids=lambda c: "%s-d%d" % c[:2])
def test_link_prediction_ranks_match_float64(case):
    """Tester.run_link_prediction on kg_small: every query's raw and filtered rank equal to the rank computed from the
    float64 score rows unless its row holds a candidate within tol(D) relative of the truth (at most 2 % of the queries:
    test_wide_reference_cpu.py); the metrics are those of the reported ranks. The type-constrained ranking, the
    Validator and triple classification run on the same model."""
    from openke.config import Tester, Validator
    from openke.data import TestDataLoader
    model, D, p, nf, _ = case
    test_dl = TestDataLoader(KG_SMALL, "link")
    tabs = wc.lp_tables(case, test_dl.get_ent_tot(), test_dl.get_rel_tot())
    kge = _model(tabs, {"model": model, "dim": D, "p_norm": p, "norm_flag": nf})
    tester = Tester(model=kge, data_loader=test_dl, use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    ranks = [np.asarray(x, dtype=np.int64) for x in tester.last_ranks]
    h, t, r = test_dl.eval_triples()
    rows_h, rows_t = wc.lp_rows64(case, tabs, h, t, r)
    all_tr = [np.concatenate(x) for x in zip(*(oracle.read_triples(KG_SMALL + f)
                                              for f in ("test2id.txt", "train2id.txt", "valid2id.txt")))]
    want = wc.ranks_from_rows(rows_h, rows_t, h, t, r, set(zip(*(x.tolist() for x in all_tr))))
    near = wc.lp_near_ties(case, rows_h, rows_t, h, t)
    assert near.any(axis=0).mean() <= 0.02
    differ = 0
    for k in range(4):
        d = ranks[k] != want[k]
        assert not (d & ~near[k // 2]).any(), (k, np.nonzero(d & ~near[k // 2])[0][:10])
        differ += int(d.sum())
    print("%s d%d: %d ranks differ, %d (query, side) pairs excused" % (model, D, differ, int(near.sum())))
    metrics_match_ranks(res, tester.last_ranks)
    assert np.isfinite(np.asarray(tester.run_link_prediction(type_constrain=True), dtype=np.float64)).all()
    hit10 = Validator(model=kge, data_loader=TestDataLoader(KG_SMALL, "link", mode="valid")).valid()
    assert 0.0 <= hit10 <= 1.0
    acc, thr = Tester(model=kge, data_loader=TestDataLoader(KG_SMALL, "classification"),
                      use_gpu=True).run_triple_classification()
    assert 0.0 <= acc <= 1.0 and np.isfinite(thr)


# ------------------------------------------------------------------ 8. the example's configuration
def test_example_configuration_runs_and_checkpoints(tmp_path):
    """examples/train_transe_WN18_adv_sigmoidloss.py on kg_small: cross sampling, 64 negatives, TransE at dim 1024
    (p_norm 1, no normalisation, margin 6), SigmoidLoss(adv_temperature=1), Adam at 2e-5: two epochs with finite
    losses, the sampler streams where the oracle's are, a checkpoint round trip bit-equal."""
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import SigmoidLoss
    from openke.module.model import TransE
    from openke.module.strategy import NegativeSampling
    threads, bs, neg, seed, epochs = 8, 100, 64, 31, 2
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=bs, threads=threads, sampling_mode="cross", bern_flag=0,
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
    nb = dl.nbatches
    torch.manual_seed(5)
    kge = TransE(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=1024, p_norm=1, norm_flag=False, margin=6.0)
    ns = NegativeSampling(model=kge, loss=SigmoidLoss(adv_temperature=1), batch_size=dl.get_batch_size(),
                          regul_rate=0.0)
    tr = Trainer(model=ns, data_loader=dl, train_times=epochs, alpha=2e-5, use_gpu=True, opt_method="adam")
    tr.run()
    assert not tr.last_run_fused
    assert len(tr.epoch_losses) == epochs and np.isfinite(tr.epoch_losses).all()
    assert np.isfinite(tr.last_step_losses).all()
    assert tr.optimizer.step == epochs * nb
    assert (tr.optimizer.exp_avg_sq[0] > 0).any()
    kg = oracle.KG.load(KG_SMALL)
    st = oracle.GlibcRand(seed).rand_reset(threads)
    modes = call_modes("c" * (epochs * nb + 1))
    for mode in modes:
        h, t, r, _ = kg.sample_ex(st, threads, bs, neg, 0, mode, 0, 1)
    dl.cross_sampling()
    np.testing.assert_array_equal(dl.batch_h, h)
    np.testing.assert_array_equal(dl.batch_t, t)
    np.testing.assert_array_equal(dl.batch_r, r)
    data = {"batch_h": h[:64], "batch_t": t[:64], "batch_r": r[:64], "mode": "normal"}
    before = kge.predict(data)
    path = os.path.join(str(tmp_path), "transe.ckpt")
    kge.save_checkpoint(path)
    torch.manual_seed(99)
    fresh = TransE(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=1024, p_norm=1, norm_flag=False,
                   margin=6.0).cuda()
    assert not np.array_equal(fresh.predict(data), before)
    fresh.load_checkpoint(path)
    np.testing.assert_array_equal(fresh.predict(data), before)
    for a, b in zip(fresh.tables()[:2], kge.tables()[:2]):
        assert torch.equal(a.detach().cpu(), b.detach().cpu())


# ------------------------------------------------------------------ 9. refusals -----------------
def test_unsupported_dims_are_refused():
    """Dims 513, 514, 1028 and 2048 for TransE and TransH, and TransD at 516: PT_ENOTSUP from pt_trainer_create,
    pt_score and pt_score_rows with the rule in the message (TransD's names TransD), NativeError through the Python
    classes, every table and output bit-untouched."""
    from openke import _native
    from openke.config import Trainer
    from openke.module.loss import MarginLoss
    from openke.module.model import TransD, TransE
    from openke.module.strategy import NegativeSampling
    L = _native.lib()
    dev = torch.device("cuda", 0)
    E, R = 6, 2
    st = _native.stream()
    idx = torch.zeros(4, dtype=torch.int64, device=dev)

    def expect(rc, *words):
        assert rc == PT_ENOTSUP, (rc, L.pt_last_error().decode())
        msg = L.pt_last_error().decode()
        assert all(w in msg for w in words), msg

    for model, D, words in [(m, d, (str(d), RULE)) for m in (_native.PT_TRANSE, _native.PT_TRANSH)
                            for d in (513, 514, 1028, 2048)] + [(_native.PT_TRANSD, 516, ("516", "TransD", "1..512"))]:
        assert L.pt_model_dim_supported(D, model) == 0
        tabs = [torch.rand(rows, D, device=dev) - 0.5 for rows in (E, R, R, E, R)]
        keep = [x.clone() for x in tabs]
        d = _native.ModelDesc()
        d.model, d.p_norm, d.norm_flag, d.opt, d.lr, d.margin = model, 1, 1, _native.PT_SGD, 0.1, 2.0
        d.ent_total, d.rel_total, d.dim = E, R, D
        d.ent, d.rel = tabs[0].data_ptr(), tabs[1].data_ptr()
        if model == _native.PT_TRANSH:
            d.normv = tabs[2].data_ptr()
        if model == _native.PT_TRANSD:
            d.ent_transfer, d.rel_transfer = tabs[3].data_ptr(), tabs[4].data_ptr()
        h = ctypes.c_void_p()
        expect(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)), *words)
        assert not h.value
        out = torch.full((4,), 7.0, device=dev)
        expect(L.pt_score(ctypes.byref(d), 0, _native.ptr(idx), _native.ptr(idx), _native.ptr(idx), 4, _native.ptr(out),
                          st), *words)
        rows = torch.full((4, E), 7.0, device=dev)
        expect(L.pt_score_rows(ctypes.byref(d), 0, _native.ptr(idx), _native.ptr(idx), _native.ptr(idx), 4,
                               _native.ptr(rows), st), *words)
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (rows == 7.0).all()
        for a, b in zip(tabs, keep):
            assert torch.equal(a, b)
    batch = {"batch_h": np.array([0, 1, 2, 3]), "batch_t": np.array([1, 2, 3, 4]), "batch_r": np.array([0, 1, 0, 1]),
             "mode": "normal"}
    for kge, frag in ((TransE(E, R, dim=514), RULE), (TransD(E, R, dim_e=516, dim_r=516), "TransD")):
        w0 = [t.detach().clone() for t in kge.tables() if t is not None]
        tr = Trainer(model=NegativeSampling(model=kge, loss=MarginLoss(margin=1.0), batch_size=2), data_loader=None,
                     train_times=0, alpha=0.1, use_gpu=True)
        with pytest.raises(_native.NativeError, match=frag):
            tr.train_one_step(batch)
        with pytest.raises(_native.NativeError, match=frag):
            kge.predict(batch)
        for a, b in zip(w0, [t for t in kge.tables() if t is not None]):
            assert torch.equal(a, b.detach().cpu())


def test_neg_beyond_the_score_buffer_is_refused_at_dim_1024():
    """k_step_adv's 64 KB of LDS hold a group's transpose row (1,024 floats at dim 1024) beside its scores: neg up to
    15,360 trains, one more is PT_ENOTSUP with the limit in the message and the tables untouched."""
    from openke import _native
    from openke.config import Trainer
    from openke.module.loss import SigmoidLoss
    from openke.module.model import TransE
    from openke.module.strategy import NegativeSampling
    torch.manual_seed(1)
    kge = TransE(6, 2, dim=1024)
    tr = Trainer(model=NegativeSampling(model=kge, loss=SigmoidLoss(adv_temperature=1.0), batch_size=1),
                 data_loader=None, train_times=0, alpha=0.1, use_gpu=True)
    limit = 16384 - 1024

    def batch(n):
        return {"batch_h": np.zeros(n + 1, dtype=np.int64), "batch_t": np.ones(n + 1, dtype=np.int64),
                "batch_r": np.zeros(n + 1, dtype=np.int64), "mode": "normal"}

    assert np.isfinite(tr.train_one_step(batch(limit)))
    w0 = [t.detach().clone() for t in kge.tables()[:2]]
    with pytest.raises(_native.NativeError, match="too large.*max %d" % limit):
        tr.train_one_step(batch(limit + 1))
    for a, b in zip(w0, kge.tables()[:2]):
        assert torch.equal(a, b.detach())


def test_fused_query_answers_what_the_run_does():
    """pt_trainer_fused_supported at the dims the fused run has always taken: 1 for plain TransE / TransH at small and
    large neg, 0 under a non-default loss, Adam or TransD, where pt_trainer_run answers PT_ENOTSUP."""
    from openke import _native
    L = _native.lib()
    dev = torch.device("cuda", 0)
    E, R, D = 50, 4, 20
    tabs = [torch.rand(rows, D, device=dev) - 0.5 for rows in (E, R, R, E, R)]

    def trainer(model, opt, dim=D):
        d = _native.ModelDesc()
        d.model, d.p_norm, d.norm_flag, d.opt, d.lr, d.margin = model, 1, 1, opt, 0.1, 2.0
        d.ent_total, d.rel_total, d.dim = E, R, dim
        d.ent, d.rel = tabs[0].data_ptr(), tabs[1].data_ptr()
        d.normv = tabs[2].data_ptr() if model == _native.PT_TRANSH else None
        if model == _native.PT_TRANSD:
            d.ent_transfer, d.rel_transfer = tabs[3].data_ptr(), tabs[4].data_ptr()
        h = ctypes.c_void_p()
        _native.check(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)))
        return h

    for model in (_native.PT_TRANSE, _native.PT_TRANSH):
        t = trainer(model, _native.PT_SGD)
        assert [L.pt_trainer_fused_supported(t, 40, n) for n in (1, 3, 4, 25, 300)] == [1] * 5
        assert L.pt_trainer_fused_supported(t, 0, 3) == 0 and L.pt_trainer_fused_supported(t, 40, 0) == 0
        if model == _native.PT_TRANSE:
            ld = _native.LossDesc()
            ld.kind = _native.PT_LOSS_SIGMOID
            _native.check(L.pt_trainer_set_loss(t, ctypes.byref(ld)))
            assert L.pt_trainer_fused_supported(t, 40, 3) == 0
        L.pt_trainer_free(t)
    for model, opt in ((_native.PT_TRANSE, _native.PT_ADAM), (_native.PT_TRANSD, _native.PT_SGD)):
        t = trainer(model, opt)
        assert L.pt_trainer_fused_supported(t, 40, 25) == 0
        L.pt_trainer_free(t)
    assert L.pt_trainer_fused_supported(None, 40, 25) == 0
