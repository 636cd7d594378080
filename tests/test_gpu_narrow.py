"""The one-float row kernels at the shapes and instances no other test executes, on the GPU, against the float64
references (adv_reference.py, lp_reference.py, transd_reference.py):

  A. k_step_sampled + k_sample_csr + k_apply through pt_trainer_step with in-kernel sampling on kg_small, one to two
     teacher-forced steps per case, at every (G, KCH) one-float row shape and every (NCH, S) column of PT_SSHAPES for
     TransE and TransH (narrow_cases.SAMPLED_CASES; test_narrow_reference_cpu.py prints which instance each selects);
  B. k_score, k_score_queries, k_lp_bases, k_step + k_apply, k_step_adv, k_apply_adam and the three TransD kernels at
     row shapes (2,1,1), (4,1,1), (16,1,1), (64,1,4) and (64,1,8): dims 2, 3, 13, 130, 255, 257 and 511.

Tolerances are narrow_cases.py's: the project's rules with the deviation tables measured on the CPU
(test_narrow_reference_cpu.py, which also asserts the input conditions of every case here). No cell is excluded.
Every test prints its observed maxima beside its bound."""
import ctypes

import numpy as np
import pytest
import torch

import adv_reference as ar
import narrow_cases as nc
import transd_cases as tc
import transd_reference as tr
import wide_cases as wc
from conftest import KG_SMALL
from lp_reference import lp_min64, lp_scores64
from test_gpu_lp_values import _check as _check_lp, _run as _run_lp, _universe_array

pytestmark = pytest.mark.gpu

B1, B2 = 0.9, 0.999


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
    worst = 0.0
    for i, w in enumerate(want):
        dev = float(np.abs((tabs[i].astype(np.float64) - got[i].astype(np.float64)) - w).max())
        print("%s table %d: max |delta_gpu - delta_ref64| %.3e (tol %.3e, |g|max %.3e)" % (tag, i, dev, tol, gmax))
        assert dev <= tol, (tag, i, dev, tol)
        worst = max(worst, dev)
    return worst


# ------------------------------------------------------------------ A. the sampled step ---------
@pytest.mark.parametrize("case", nc.SAMPLED_CASES, ids=nc.sampled_name)
def test_sampled_step_matches_float64(case):
    """pt_trainer_step with in-kernel sampling under SGD lr 1 (the table delta is the gradient) or Adagrad lr 1 from a
    given state_sum in [1, 2) (|d delta / d g| <= 1 there). Every step starts from the case's tables and the oracle's
    sampler streams, its batch is the oracle's sampling(): every cell of every table, norm_vector included, within the
    gradient bound of the float64 reference, the loss to rtol 1e-5, every row no slot names bit-identical, and the
    streams end where the oracle's do."""
    from openke import _native
    from openke.module.model import TransE, TransH
    model, D, p, nf, opt, bs, neg, bern, filt, steps = case
    b = nc.build_sampled(case)
    cfg, name = b["cfg"], b["name"]
    tabs = [x for x in b["tabs"] if x is not None]
    L = _native.lib()
    E, R = tabs[0].shape[0], tabs[1].shape[0]
    kge = (TransE if model == "TransE" else TransH)(E, R, dim=D, p_norm=p, norm_flag=nf).cuda()
    devt = [t for t in kge.tables() if t is not None]
    ada = opt == "adagrad"
    state = [s for s in nc.adagrad_state(b["tabs"]) if s is not None] if ada else None
    dacc = [torch.zeros_like(t) for t in devt] if ada else []
    accs = tuple(dacc) + (None,) * (3 - len(dacc)) if ada else (None, None, None)
    desc = kge.native_desc(_native.PT_ADAGRAD if ada else _native.PT_SGD, 1.0, cfg["loss_margin"], accs)
    g, smp, trn = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    _native.check(L.pt_graph_load(KG_SMALL.encode(), ctypes.byref(g)))
    st0 = np.ascontiguousarray(b["states"][0])
    _native.check(L.pt_sampler_create(g, nc.SAMPLER_THREADS, st0.ctypes.data, ctypes.byref(smp)))
    _native.check(L.pt_trainer_create(ctypes.byref(desc), ctypes.byref(trn)))
    try:
        loss = torch.zeros(1, device="cuda")
        for k, s in enumerate(b["steps"]):
            with torch.no_grad():
                for d_, h_ in zip(devt + dacc, tabs + (state or [])):
                    d_.copy_(torch.from_numpy(h_))
            st = np.ascontiguousarray(b["states"][k])
            _native.check(L.pt_sampler_set_seeds(smp, st.ctypes.data))
            loss.zero_()
            _native.check(L.pt_trainer_step(trn, smp, bs, neg, bern, filt, None, None, None, _native.ptr(loss),
                                            _native.stream()))
            got = [t.detach().cpu().numpy().copy() for t in devt]
            got_loss = float(loss.item())
            nxt = np.zeros(nc.SAMPLER_THREADS, dtype=np.uint64)
            _native.check(L.pt_sampler_get_seeds(smp, nxt.ctypes.data))
            np.testing.assert_array_equal(nxt, b["states"][k + 1])
            want = s["grads"] if not ada else [nc.adagrad_delta(state[i], gr) for i, gr in enumerate(s["grads"])]
            gmax = s["aux"]["gmax"]
            _check_delta("%s step %d" % (name, k), tabs, got, want, nc.grad_tol(gmax, cfg), gmax)
            print("%s step %d loss gpu %.9g ref %.9g" % (name, k, got_loss, s["loss"]))
            assert abs(got_loss - s["loss"]) <= 1e-5 * abs(s["loss"]), (got_loss, s["loss"])
            h, t, r = s["hrt"]
            free_e = np.setdiff1d(np.arange(E), np.concatenate([h, t]))
            free_r = np.setdiff1d(np.arange(R), r)
            np.testing.assert_array_equal(got[0][free_e], tabs[0][free_e])
            for i in range(1, len(tabs)):
                np.testing.assert_array_equal(got[i][free_r], tabs[i][free_r])
            if ada:
                for i, a in enumerate(dacc):   # and their Adagrad state
                    free = free_e if i == 0 else free_r
                    np.testing.assert_array_equal(a.cpu().numpy()[free], state[i][free])
    finally:
        torch.cuda.synchronize()
        L.pt_trainer_free(trn)
        L.pt_sampler_free(smp)
        L.pt_graph_free(g)


# ------------------------------------------------------------------ B1. scores -------------------
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
@pytest.mark.parametrize("D", nc.NARROW_DIMS)
def test_scores_match_float64(D, model):
    """predict in its three modes (k_score) and pt_score_rows on both sides (k_score_queries), p 1 / 2 with and without
    normalisation: every cell within tol(D) of the float64 reference."""
    tol = nc.score_tol(D)
    worst = 0.0
    for p in (1, 2):
        for nf in (True, False):
            tabs, batches = nc.score_case(model, D, p, nf)
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


@pytest.mark.parametrize("model", ["TransE", "TransH"])
@pytest.mark.parametrize("D", nc.NARROW_DIMS)
def test_lp_min_scores_match_float64(D, model):
    """pt_lp_min_scores (k_lp_bases at the one-float shape, then the scan) on one universe of 65 local entities, 29
    pairs of mixed sides: every finite cell of the rows and of the tuple row within tol(D), the finite mask the
    reference's (test_gpu_lp_values.test_scores_match_fp64 at these dims)."""
    from openke import _native as n
    tol = nc.score_tol(D)
    worst = 0.0
    for p in (1, 2):
        for nf in (1, 0):
            u, pairs = nc.lp_case(model, D, p, bool(nf))
            uni = {"h": u, "d": {k: torch.from_numpy(v).cuda() for k, v in u.items() if v is not None}}
            ua = _universe_array(n, [uni])
            rows, tup = _run_lp(n, ua, model, p, nf, pairs, nc.LP_GLOBAL_E, nc.LP_KEYS)
            ref_rows, ref_tup = lp_min64([u], pairs, nc.LP_GLOBAL_E, nc.LP_KEYS, model, p, nf)
            what = "narrow D %d %s p %d nf %d" % (D, model, p, nf)
            worst = max(worst, _check_lp(what + " rows", rows.cpu().numpy(), ref_rows, np.full(ref_rows.shape, tol)),
                        _check_lp(what + " tuple", tup.cpu().numpy(), ref_tup, np.full(ref_tup.shape, tol)))
    print("%s D %d: worst |gpu - ref64| / max(1, ref64) %.3e (tol %.3e)" % (model, D, worst, tol))


# ------------------------------------------------------------------ B2. the plain step -----------
@pytest.mark.parametrize("case", nc.PLAIN_CASES, ids=lambda c: c[0])
def test_plain_step_gradient_parity(case):
    """k_step + k_apply on an external batch under SGD lr 1 or Adagrad lr 1 from a given state_sum in [1, 2): every
    cell of every table within the gradient bound, the loss to rtol 1e-5, the rows no slot names bit-identical
    (test_gpu_wide.test_plain_step_gradient_parity at the one-float shapes)."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, hrt, cfg = nc.build_plain(case)
    tabs = [x for x in tabs if x is not None]
    bs, opt = cfg["batch_size"], case[7]
    want_loss, grads, aux = ar.loss_and_grads(tabs, *hrt, bs, cfg)
    kge, trn = _trainer(tabs + [None], cfg, opt, 1.0)
    want = grads
    if opt == "adagrad":
        trn.optimizer = NativeOptimizer(_native.PT_ADAGRAD, 1.0, kge.tables())
        state = nc.adagrad_state(tabs)
        for s, x in zip([s for s in trn.optimizer.state_sum if s is not None], state):
            s.copy_(torch.from_numpy(x))
        want = [nc.adagrad_delta(state[i], g) for i, g in enumerate(grads)]
    loss = trn.train_one_step(wc.as_batch(hrt))
    got = _tables(kge)
    _check_delta(case[0], tabs, got, want, nc.grad_tol(aux["gmax"], cfg), aux["gmax"])
    print("%s loss gpu %.9g ref %.9g" % (case[0], loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
    np.testing.assert_array_equal(got[0][wc.FREE_ENT], tabs[0][wc.FREE_ENT])
    for i in range(1, len(tabs)):
        np.testing.assert_array_equal(got[i][wc.FREE_REL], tabs[i][wc.FREE_REL])


# ------------------------------------------------------------------ B3. the weighted step, Adam --
@pytest.mark.parametrize("case", nc.ADV_CASES, ids=lambda c: c[0])
def test_weighted_step_gradient_parity(case):
    """k_step_adv (TransE): the four loss families at dims 130 and 257 with K = 3 and K = 70 under SGD lr 1: finite,
    every cell of both tables within the gradient bound, the loss to rtol 1e-5."""
    tabs, batch, cfg = wc.build_adv(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = ar.loss_and_grads(tabs, *wc.expanded(batch, bs), bs, cfg)
    kge, trn = _trainer(tabs, cfg, "sgd", 1.0)
    loss = trn.train_one_step(batch)
    got = _tables(kge)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in got)
    _check_delta(case[0], tabs, got, grads, nc.grad_tol(aux["gmax"], cfg), aux["gmax"])
    print("%s loss gpu %.9g ref %.9g" % (case[0], loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)


@pytest.mark.parametrize("case", nc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_three_steps_from_given_state(case):
    """k_apply_adam after k_step_adv (TransE) and k_step (TransH) at dims 13, 130 and 257 under test_gpu_adv.py's
    bounds: after every step exp_avg / exp_avg_sq within (1 - b1) tol / (1 - b2) 2 |g|max tol of the float64 update at
    the GPU's own pre-step state, every weight the float64 update formula at the GPU's own new moments (4 ulp of w +
    1e-6 |delta|); the row touched in step 1 only keeps moving, the row never touched stays put with zero state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, batches, cfg, (m0, v0), lr, step0 = wc.build_adam(case)
    bs = cfg["batch_size"]
    kge, trn = _trainer(tabs, cfg, "adam", lr)
    trn.optimizer = NativeOptimizer(_native.PT_ADAM, lr, kge.tables())
    opt = trn.optimizer
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
        loss = trn.train_one_step(batch)
        assert opt.step == step0 + s + 1
        assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
        w2 = _tables(kge)
        m2, v2 = state()
        tol = nc.grad_tol(aux["gmax"], cfg)
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


# ------------------------------------------------------------------ B4. TransD -------------------
def _transd(tabs, cfg):
    from openke.module.model import TransD
    kge = TransD(tabs[0].shape[0], tabs[1].shape[0], dim_e=cfg["dim"], dim_r=cfg["dim"], p_norm=cfg["p_norm"],
                 norm_flag=cfg["norm_flag"])
    for name, x in zip(tr.TABLES, tabs):
        getattr(kge, name).weight.data.copy_(torch.from_numpy(np.asarray(x)))
    return kge


@pytest.mark.parametrize("D", nc.TRANSD_DIMS)
def test_transd_scores_match_float64(D):
    """pt_score in the three modes (through predict) and pt_score_rows on both sides at dims 13, 130 and 257."""
    from openke import _native
    tol = nc.transd_score_tol(D)
    worst = 0.0
    for p in (1, 2):
        for nf in (True, False):
            tabs, batches, cfg = tr.score_case(D, p, nf)
            kge = _transd(tabs, cfg).cuda()
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
                rows = _rows(kge, side, h[:nq], t[:nq], r[:nq])
                err = np.abs(rows - ref) / np.maximum(1.0, ref)
                worst = max(worst, float(err.max()))
                assert (err <= tol).all(), (D, p, nf, side, "rows", float(err.max()), tol)
    assert _native.lib().pt_model_dim_supported(D, _native.PT_TRANSD) == 1
    print("TransD D %d: worst |gpu - ref64| / max(1, ref64) %.3e (tol %.3e)" % (D, worst, tol))


@pytest.mark.parametrize("case", nc.TRANSD_CASES, ids=lambda c: c[0])
def test_transd_gradient_parity_sgd(case):
    """k_step_transd + k_apply (twice) under SGD lr 1 with transd_cases' builders: every cell of all four tables
    within the gradient bound, the loss to rtol 1e-5, the entity and relation no slot names bit-identical."""
    from openke.config import Trainer
    from openke.module.loss import MarginLoss
    from openke.module.strategy import NegativeSampling
    tabs, hrt, cfg, mode = tc.build(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = tr.loss_and_grads(tabs, *hrt, bs, cfg, mode)
    kge = _transd(tabs, cfg)
    ns = NegativeSampling(model=kge, loss=MarginLoss(margin=cfg["loss_margin"]), batch_size=bs)
    ns.cuda()
    trn = Trainer(model=ns, data_loader=None, train_times=0, alpha=1.0, use_gpu=True, opt_method="sgd")
    loss = trn.train_one_step(tc.as_batch(hrt, bs, mode))
    got = _tables(kge)
    _check_delta(case[0], tabs, got, grads, nc.grad_tol(aux["gmax"], cfg), aux["gmax"])
    print("%s loss gpu %.9g ref %.9g" % (case[0], loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
    for i, row in ((0, tc.FREE_ENT), (2, tc.FREE_ENT), (1, tc.FREE_REL), (3, tc.FREE_REL)):
        np.testing.assert_array_equal(got[i][row], tabs[i][row])
