"""The weighted losses (SigmoidLoss, self-adversarial weights, the model's own margin: k_step_adv) and dense Adam
(k_apply_adam) on the GPU against the float64 reference tests/adv_reference.py.

Gradient parity runs SGD at lr 1 on explicit batches (adv_cases.py), so the table delta is the gradient:
    |delta_gpu - delta_ref64| <= tol = min(1e-5, max(4 * 2^-23 * max(1, |g|max), 4 * GRAD_DEV[family]))
for every cell of both tables (4 for the other summation order, GRAD_DEV the reference implementation's own float32
deviation from the float64 form, measured in test_adv_reference_cpu.py), and the loss to rtol 1e-5. The input
conditions of the seeds (no v component within 1e-6 of zero under p = 1, no hinge argument within 1e-5 of -m) are
asserted on the CPU in test_adv_reference_cpu.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import adv_cases
import adv_reference as ar
import oracle
from conftest import KG_SMALL
from helpers import golden, load
from test_oracle import call_modes

pytestmark = pytest.mark.gpu

B1, B2 = 0.9, 0.999


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible HIP device"


def _tol(gmax, cfg):
    return min(1e-5, max(4 * 2.0 ** -23 * max(1.0, gmax), 4 * ar.GRAD_DEV[ar.family(cfg)]))


def _trainer(tabs, cfg, opt, lr):
    """(kge, Trainer) for a model holding the given tables, on the GPU."""
    from openke.config import Trainer
    from openke.module.loss import MarginLoss, SigmoidLoss
    from openke.module.model import TransE, TransH
    from openke.module.strategy import NegativeSampling
    E, R = tabs[0].shape[0], tabs[1].shape[0]
    if cfg["model"] == "TransH":
        kge = TransH(E, R, dim=cfg["dim"], p_norm=cfg["p_norm"], norm_flag=cfg["norm_flag"])
        kge.norm_vector.weight.data.copy_(torch.from_numpy(tabs[2]))
    else:
        kge = TransE(E, R, dim=cfg["dim"], p_norm=cfg["p_norm"], norm_flag=cfg["norm_flag"],
                     margin=cfg["model_margin"])
    kge.ent_embeddings.weight.data.copy_(torch.from_numpy(tabs[0]))
    kge.rel_embeddings.weight.data.copy_(torch.from_numpy(tabs[1]))
    if cfg["loss"] == "sigmoid":
        loss = SigmoidLoss(adv_temperature=cfg["adv_temperature"])
    else:
        loss = MarginLoss(adv_temperature=cfg["adv_temperature"], margin=cfg["loss_margin"])
    ns = NegativeSampling(model=kge, loss=loss, batch_size=cfg["batch_size"])
    ns.cuda()
    return kge, Trainer(model=ns, data_loader=None, train_times=0, alpha=lr, use_gpu=True, opt_method=opt)


def _tables(kge):
    return [None if t is None else t.detach().cpu().numpy().copy() for t in kge.tables()]


def _expanded(batch, bs):
    return ar.expand_batch(batch["batch_h"], batch["batch_t"], batch["batch_r"], batch["mode"], bs)


@pytest.mark.parametrize("case", adv_cases.GRAD_CASES, ids=lambda c: c[0])
def test_gradient_parity_sgd(case):
    tabs, batch, cfg = adv_cases.build(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = ar.loss_and_grads(tabs, *_expanded(batch, bs), bs, cfg)
    kge, tr = _trainer(tabs, cfg, "sgd", 1.0)
    loss = tr.train_one_step(batch)
    got = _tables(kge)
    tol = _tol(aux["gmax"], cfg)
    for i in range(2):
        dev = float(np.abs((tabs[i].astype(np.float64) - got[i].astype(np.float64)) - grads[i]).max())
        print("%s table %d: max |delta_gpu - delta_ref64| %.3e (tol %.3e, |g|max %.3e)" % (case[0], i, dev, tol,
                                                                                         aux["gmax"]))
        assert dev <= tol, (case[0], i, dev, tol)
    print("%s loss gpu %.9g ref %.9g" % (case[0], loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)


def test_gradient_parity_adagrad():
    """The same step through Adagrad (k_apply) from a given state_sum in [1, 2): |d delta / d g| <= 1 there, so the
    gradient bound holds for the delta."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    case = adv_cases.ADAGRAD_CASE
    tabs, batch, cfg = adv_cases.build(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = ar.loss_and_grads(tabs, *_expanded(batch, bs), bs, cfg)
    kge, tr = _trainer(tabs, cfg, "adagrad", 1.0)
    tr.optimizer = NativeOptimizer(_native.PT_ADAGRAD, 1.0, kge.tables())
    rng = np.random.default_rng(77)
    state = [rng.uniform(1, 2, size=t.shape).astype(np.float32) for t in tabs[:2]]
    for s, x in zip(tr.optimizer.state_sum, state):
        s.copy_(torch.from_numpy(x))
    loss = tr.train_one_step(batch)
    got = _tables(kge)
    tol = _tol(aux["gmax"], cfg)
    for i in range(2):
        want = grads[i] / (np.sqrt(state[i].astype(np.float64) + grads[i] ** 2) + 1e-10)
        dev = float(np.abs((tabs[i].astype(np.float64) - got[i].astype(np.float64)) - want).max())
        print("adagrad table %d: max |delta_gpu - delta_ref64| %.3e (tol %.3e)" % (i, dev, tol))
        assert dev <= tol, (i, dev, tol)
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)


def test_stability_large_distances_high_temperature():
    """Distances around 30 at temperature 40 on unnormalised rows scaled by 8: finite, and within tol of the float64
    reference, every cell of both tables, as in the parity cases."""
    case = adv_cases.STABILITY_CASE
    tabs, batch, cfg = adv_cases.build(case)
    bs = cfg["batch_size"]
    want_loss, grads, aux = ar.loss_and_grads(tabs, *_expanded(batch, bs), bs, cfg)
    kge, tr = _trainer(tabs, cfg, "sgd", 1.0)
    loss = tr.train_one_step(batch)
    got = _tables(kge)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in got[:2])
    tol = _tol(aux["gmax"], cfg)
    for i in range(2):
        dev = float(np.abs((tabs[i].astype(np.float64) - got[i].astype(np.float64)) - grads[i]).max())
        print("stability table %d: max |delta_gpu - delta_ref64| %.3e (tol %.3e, |g|max %.3e)" % (i, dev, tol,
                                                                                                aux["gmax"]))
        assert dev <= tol, (i, dev, tol)
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)


@pytest.mark.parametrize("case", adv_cases.ADAM_CASES, ids=lambda c: c[0])
def test_adam_three_steps_from_given_state(case):
    """After every step: exp_avg / exp_avg_sq within (1 - b1) tol / (1 - b2) 2 |g|max tol of the float64 update at
    the GPU's own pre-step state, every weight the float64 update formula at the GPU's own new moments (4 ulp of w
    + 1e-6 |delta|); the row touched in step 1 only keeps moving, the row never touched stays put with zero state."""
    from openke import _native
    from openke.config.Trainer import NativeOptimizer
    tabs, batches, cfg, (m0, v0), lr, step0 = adv_cases.build_adam(case)
    bs = cfg["batch_size"]
    kge, tr = _trainer(tabs, cfg, "adam", lr)
    tr.optimizer = NativeOptimizer(_native.PT_ADAM, lr, kge.tables())
    opt = tr.optimizer
    for dst, src in zip(opt.exp_avg + opt.exp_avg_sq, m0 + v0):
        if src is not None:
            dst.copy_(torch.from_numpy(src))
    opt.step = step0
    idx = [i for i in range(3) if tabs[i] is not None]

    def state():
        return ([None if x is None else x.detach().cpu().numpy().copy() for x in opt.exp_avg],
                [None if x is None else x.detach().cpu().numpy().copy() for x in opt.exp_avg_sq])

    w = _tables(kge)
    m, v = state()
    for s, batch in enumerate(batches):
        want_loss, grads, aux = ar.loss_and_grads([w[i] for i in idx], *_expanded(batch, bs), bs, cfg)
        if cfg["loss"] == "margin":
            assert aux["hinge_gap"] >= 1e-5
        if cfg["p_norm"] == 1:
            assert aux["min_abs_v"] >= 1e-6
        loss = tr.train_one_step(batch)
        assert opt.step == step0 + s + 1
        assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
        w2 = _tables(kge)
        m2, v2 = state()
        tol = _tol(aux["gmax"], cfg)
        for j, i in enumerate(idx):
            _, mr, vr = ar.adam_update(w[i], m[i], v[i], grads[j], lr, opt.step)
            dm, dv = float(np.abs(m2[i] - mr).max()), float(np.abs(v2[i] - vr).max())
            print("%s step %d table %d: |m - ref| %.3e (bound %.3e), |v - ref| %.3e (bound %.3e)"
                  % (case[0], s, i, dm, (1 - B1) * tol, dv, (1 - B2) * 2 * aux["gmax"] * tol))
            assert dm <= (1 - B1) * tol
            assert dv <= (1 - B2) * 2 * aux["gmax"] * tol
            wr = ar.adam_weights(w[i], m2[i], v2[i], lr, opt.step)
            bound = 4 * np.spacing(np.abs(w[i])).astype(np.float64) + 1e-6 * np.abs(wr - w[i])
            assert (np.abs(w2[i].astype(np.float64) - wr) <= bound).all(), (case[0], s, i)
        # entity 6: touched in step 1 only, still moving; entity 7: never touched
        assert (w2[0][6] != w[0][6]).any(), "row 6 must move in step %d" % (s + 1)
        assert s > 0 or (grads[0][6] != 0).any()
        assert s == 0 or not (grads[0][6] != 0).any()
        assert (w2[0][7] == tabs[0][7]).all() and not m2[0][7].any() and not v2[0][7].any()
        w, m, v = w2, m2, v2


@pytest.mark.parametrize("path", golden("adv_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_adam_matches_reference_trajectories(path):
    """The reference implementation's 10-step Adam runs: losses to rtol 1e-4, every table element within Adam's
    per-step bound for two trajectories (a sanity cap: the parity proof is the test above)."""
    z = load(path)
    cfg = ar.golden_cfg(z)
    lr, steps = float(z["lr"]), int(z["steps"])
    tabs = [None if x is None else np.array(x) for x in ar.golden_tables(z, "init")]
    kge, tr = _trainer(tabs, cfg, "adam", lr)
    for s in range(steps):
        batch = {"batch_h": z["b%d_h" % s], "batch_t": z["b%d_t" % s], "batch_r": z["b%d_r" % s],
                 "mode": str(z["modes"][s])}
        loss = tr.train_one_step(batch)
        assert abs(loss - float(z["losses"][s])) <= 1e-4 * abs(float(z["losses"][s])), (s, loss, float(z["losses"][s]))
    assert tr.optimizer.step == steps
    cap = 2 * steps * lr * (1 - B1) / np.sqrt(1 - B2)
    for got, want in zip(_tables(kge), ar.golden_tables(z, "final")):
        if want is not None:
            assert float(np.abs(got - want).max()) <= cap


def test_example_shaped_run_and_link_prediction():
    """Trainer.run() in the shape of examples/train_transe_WN18_adv_sigmoidloss.py on kg_small (cross sampling,
    TransE with its own margin, SigmoidLoss(adv_temperature=1), adam), then Tester.run_link_prediction."""
    from openke.config import Tester, Trainer
    from openke.data import TestDataLoader, TrainDataLoader
    from openke.module.loss import SigmoidLoss
    from openke.module.model import TransE
    from openke.module.strategy import NegativeSampling
    threads, bs, neg, seed, epochs = 8, 150, 8, 31, 3
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=bs, threads=threads, sampling_mode="cross", bern_flag=0,
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
    nb = dl.nbatches
    torch.manual_seed(5)
    kge = TransE(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=32, p_norm=1, norm_flag=False, margin=6.0,
                 epsilon=2.0)
    ns = NegativeSampling(model=kge, loss=SigmoidLoss(adv_temperature=1), batch_size=dl.get_batch_size())
    tr = Trainer(model=ns, data_loader=dl, train_times=epochs, alpha=1e-2, use_gpu=True, opt_method="adam")
    tr.run()
    assert len(tr.epoch_losses) == epochs and np.isfinite(tr.epoch_losses).all()
    assert np.isfinite(tr.last_step_losses).all()
    assert tr.epoch_losses[-1] < tr.epoch_losses[0]
    assert tr.optimizer.step == epochs * nb
    assert (tr.optimizer.exp_avg_sq[0] > 0).any()
    # the sampler streams and the cross flag advanced by exactly epochs * nbatches loader calls
    kg = oracle.KG.load(KG_SMALL)
    st = oracle.GlibcRand(seed).rand_reset(threads)
    modes = call_modes("c" * (epochs * nb + 1))
    for mode in modes:
        h, t, r, _ = kg.sample_ex(st, threads, bs, neg, 0, mode, 0, 1)
    d = dl.cross_sampling()
    np.testing.assert_array_equal(dl.batch_h, h)
    np.testing.assert_array_equal(dl.batch_t, t)
    np.testing.assert_array_equal(dl.batch_r, r)
    assert d["mode"] == {-1: "head_batch", 1: "tail_batch"}[modes[-1]]
    tester = Tester(model=kge, data_loader=TestDataLoader(KG_SMALL, "link"), use_gpu=True)
    res = tester.run_link_prediction(type_constrain=False)
    assert np.isfinite(np.asarray(res, dtype=np.float64)).all()


def _small(cls_name="TransE", **kw):
    from openke.module.model import TransE, TransH
    torch.manual_seed(1)
    return (TransE if cls_name == "TransE" else TransH)(6, 2, dim=8, **kw)


def _ns(kge, loss, **kw):
    from openke.module.strategy import NegativeSampling
    return NegativeSampling(model=kge, loss=loss, batch_size=2, **kw)


BATCH = {"batch_h": np.array([0, 1, 2, 3]), "batch_t": np.array([1, 2, 3, 4]), "batch_r": np.array([0, 1, 0, 1]),
         "mode": "normal"}


def test_unsupported_python_combinations_raise():
    from openke.config import Trainer
    from openke.module.loss import MarginLoss, SigmoidLoss
    cases = [
        (_ns(_small("TransH"), SigmoidLoss(adv_temperature=1.0)), {}),                    # TransH, weighted loss
        (_ns(_small("TransH"), MarginLoss(adv_temperature=1.0)), {}),
        (_ns(_small("TransH", margin=3.0), MarginLoss()), {}),                            # TransH with a model margin
        (_ns(_small(), SigmoidLoss()), {"opt_method": "adadelta"}),                       # Adadelta
        (_ns(_small(), SigmoidLoss(), regul_rate=0.1), {}),                               # regularisation
        (_ns(_small(), SigmoidLoss()), {"deterministic": True}),                          # reference-order mode
        (_ns(_small(), MarginLoss()), {"deterministic": True, "opt_method": "adam"}),
        (_ns(_small(margin=2.0), MarginLoss()), {"deterministic": True}),
    ]
    for ns, kw in cases:
        tr = Trainer(model=ns, data_loader=None, train_times=0, alpha=0.1, use_gpu=True, **kw)
        with pytest.raises(NotImplementedError):
            tr.train_one_step(BATCH)
    for setter in ("set_lr_decay", "set_weight_decay"):
        tr = Trainer(model=_ns(_small(), SigmoidLoss(adv_temperature=1.0)), data_loader=None, train_times=0, alpha=0.1,
                     use_gpu=True, opt_method="adam")
        getattr(tr, setter)(0.1)
        with pytest.raises(NotImplementedError):
            tr.train_one_step(BATCH)


def test_unsupported_native_combinations_return_enotsup():
    """pt_trainer_run / in-kernel sampling / the reference-order mode with a non-default loss or Adam, and TransH
    with a non-default loss: PT_ENOTSUP with a message, never another kernel."""
    from openke import _native
    from openke.data import TrainDataLoader
    L = _native.lib()
    PT_ENOTSUP, PT_ESTATE = 6, 5
    dev = torch.device("cuda", 0)
    dl = TrainDataLoader(in_path=KG_SMALL, batch_size=50, threads=8, bern_flag=0, filter_flag=1, neg_ent=2,
                         random_seed=3)
    sampler = dl.device_sampler()
    E, R, D = dl.get_ent_tot(), dl.get_rel_tot(), 8
    mk = lambda rows: torch.rand(rows, D, device=dev) - 0.5
    ent, rel, nv = mk(E), mk(R), mk(R)
    losses = torch.zeros(4, device=dev)

    def trainer(model, opt):
        d = _native.ModelDesc()
        d.model, d.p_norm, d.norm_flag, d.opt, d.lr, d.margin = model, 1, 1, opt, 0.1, 2.0
        d.ent_total, d.rel_total, d.dim = E, R, D
        d.ent, d.rel = ent.data_ptr(), rel.data_ptr()
        d.normv = nv.data_ptr() if model == _native.PT_TRANSH else None
        h = ctypes.c_void_p()
        _native.check(L.pt_trainer_create(ctypes.byref(d), ctypes.byref(h)))
        return h

    def loss_desc(kind, adv=0, temp=0.0, flag=0, gamma=0.0):
        ld = _native.LossDesc()
        ld.kind, ld.adv, ld.temperature, ld.score_margin_flag, ld.score_margin = kind, adv, temp, flag, gamma
        return ld

    def expect_enotsup(rc, *words):
        assert rc == PT_ENOTSUP, rc
        msg = L.pt_last_error().decode()
        assert all(w in msg for w in words), msg

    st = _native.stream()
    # a non-default loss: no captured run, no in-kernel sampling, no reference-order mode
    for ld in (loss_desc(_native.PT_LOSS_SIGMOID), loss_desc(_native.PT_LOSS_MARGIN, adv=1, temp=1.0),
               loss_desc(_native.PT_LOSS_MARGIN, flag=1, gamma=3.0)):
        t = trainer(_native.PT_TRANSE, _native.PT_SGD)
        _native.check(L.pt_trainer_set_loss(t, ctypes.byref(ld)))
        expect_enotsup(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), "external batches")
        expect_enotsup(L.pt_trainer_step(t, sampler, 50, 2, 0, 1, None, None, None, _native.ptr(losses), st),
                       "external batches")
        _native.check(L.pt_trainer_set_deterministic(t, 1))
        h = torch.zeros(150, dtype=torch.int64, device=dev)
        expect_enotsup(L.pt_trainer_step(t, None, 50, 2, 0, 0, _native.ptr(h), _native.ptr(h), _native.ptr(h),
                                         _native.ptr(losses), st), "reference-order")
        L.pt_trainer_free(t)
    # the default loss descriptor leaves every path as it was
    t = trainer(_native.PT_TRANSE, _native.PT_SGD)
    ld = loss_desc(_native.PT_LOSS_MARGIN)
    _native.check(L.pt_trainer_set_loss(t, ctypes.byref(ld)))
    _native.check(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st))
    torch.cuda.synchronize()
    L.pt_trainer_free(t)
    # Adam: the same, and a step before pt_trainer_set_adam is a state error
    t = trainer(_native.PT_TRANSE, _native.PT_ADAM)
    expect_enotsup(L.pt_trainer_run(t, sampler, 50, 2, 0, 1, 2, _native.ptr(losses), st), "PT_ADAM")
    expect_enotsup(L.pt_trainer_step(t, sampler, 50, 2, 0, 1, None, None, None, _native.ptr(losses), st), "PT_ADAM")
    h = torch.zeros(150, dtype=torch.int64, device=dev)
    assert L.pt_trainer_step(t, None, 50, 2, 0, 0, _native.ptr(h), _native.ptr(h), _native.ptr(h),
                             _native.ptr(losses), st) == PT_ESTATE
    assert L.pt_trainer_adam_step(t) == 0
    L.pt_trainer_free(t)
    # TransH with a non-default loss
    t = trainer(_native.PT_TRANSH, _native.PT_SGD)
    ld = loss_desc(_native.PT_LOSS_SIGMOID, adv=1, temp=1.0)
    expect_enotsup(L.pt_trainer_set_loss(t, ctypes.byref(ld)), "TransE only")
    L.pt_trainer_free(t)
    torch.cuda.synchronize()


def test_neg_beyond_the_score_buffer_is_refused():
    """neg has no silent limit: what k_step_adv's LDS score buffer cannot hold is PT_ENOTSUP with a message."""
    from openke import _native
    from openke.module.loss import SigmoidLoss
    from openke.config import Trainer
    kge = _small()
    tr = Trainer(model=_ns(kge, SigmoidLoss(adv_temperature=1.0)), data_loader=None, train_times=0, alpha=0.1,
                 use_gpu=True)
    tr.model.batch_size = 1
    n = 16384 + 1
    big = {"batch_h": np.zeros(n + 1, dtype=np.int64), "batch_t": np.ones(n + 1, dtype=np.int64),
           "batch_r": np.zeros(n + 1, dtype=np.int64), "mode": "normal"}
    with pytest.raises(_native.NativeError, match="too large"):
        tr.train_one_step(big)
