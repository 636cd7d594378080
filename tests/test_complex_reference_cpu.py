"""complex_reference.py (the float64 form of ComplEx with its regulariser) against the reference implementation's own
float32 runs (tests/golden/complex_*.npz, written by tests/golden/make_golden_complex.py), the Python ComplEx, the
Python-side refusals that need no device, and the input conditions of the GPU cases of test_gpu_complex.py checked on
the CPU."""
import numpy as np
import pytest
import torch

import complex_cases as cc
import complex_reference as cr
from helpers import golden, load
from openke.module.loss import MarginLoss, SigmoidLoss, SoftplusLoss
from openke.module.model import ComplEx   # (no test of this file means anything without the model)

ALL_FIXTURES = ("complex_g*.npz", "complex_a*.npz", "complex_p*.npz", "complex_lp.npz")


def _fixtures():
    return [p for pat in ALL_FIXTURES for p in golden(pat)]


# ------------------------------------------------------------------ the reference's own runs ----
@pytest.mark.parametrize("path", golden("complex_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_gradients_match_reference_runs(path):
    """Every SGD lr 1 step of the reference: its table delta is the float64 gradient at the tables before it within
    GRAD_DEV of the case's family, its loss the float64 loss within LOSS_DEV."""
    z = load(path)
    cfg = cr.golden_cfg(z)
    assert int(z["steps"]) >= 2 and float(z["lr"]) == 1.0
    worst, lworst = cr.measure_golden_dev(z)
    print("%s: reference float32 gradient deviation %.3e (GRAD_DEV %.3e), loss %.3e (LOSS_DEV %.3e)"
          % (path.split("/")[-1], worst, cr.GRAD_DEV[cr.family(cfg)], lworst, cr.LOSS_DEV))
    assert worst <= cr.GRAD_DEV[cr.family(cfg)]
    assert lworst <= cr.LOSS_DEV


def test_golden_cases_cover_the_issue():
    """SigmoidLoss and SoftplusLoss, each with and without the temperature, regul_rate 0 and 1, normal sampling with
    one relation-corruption case, dims 5, 7, 8, 12, 16, 20."""
    seen, dims, regs, negrel = set(), set(), set(), set()
    for path in golden("complex_g*.npz"):
        cfg = cr.golden_cfg(load(path))
        assert cfg["sampling"] == "normal"
        seen.add((cfg["loss"], cfg["adv_temperature"] is not None))
        dims.add(cfg["dim"]); regs.add(cfg["regul_rate"]); negrel.add(cfg["neg_rel"] > 0)
    assert seen == {("sigmoid", True), ("sigmoid", False), ("softplus", True), ("softplus", False)}
    assert dims == {5, 7, 8, 12, 16, 20} and regs == {0.0, 1.0} and negrel == {True, False}
    z = load(golden("complex_g4.npz")[0])   # the relation corruptions are in the batch
    bs = int(z["batch_size"])
    assert (z["b0_r"][bs:].reshape(-1, bs) != z["b0_r"][:bs]).any()
    opts = {str(load(p)["optimizer"]): load(p) for p in golden("complex_a*.npz")}
    assert set(opts) == {"adagrad", "adam"}
    assert float(opts["adagrad"]["regul_rate"]) == 1.0 and int(opts["adagrad"]["bern"]) == 1
    assert all(int(z["steps"]) == 10 for z in opts.values())
    assert len(golden("complex_p*.npz")) == 3 and len(golden("complex_lp.npz")) == 1


@pytest.mark.parametrize("path", golden("complex_p*.npz"), ids=lambda p: p.split("/")[-1])
def test_predict_matches_reference(path):
    """The reference's predict (-s) in the three modes: the float64 scores within score_tol, and the float32 evaluation
    of the same forward (what SCORE_DEV measures) to two ulps."""
    z = load(path)
    tabs = cr.golden_tables(z, "")
    D = int(z["dim"])
    for mode in ("normal", "head_batch", "tail_batch"):
        h, t, r = cr.expand_predict(z[mode + "_h"], z[mode + "_t"], z[mode + "_r"], mode)
        want = z[mode + "_score"].astype(np.float64)
        ref = -cr.scores(tabs, h, t, r)
        assert (np.abs(ref - want) <= cr.score_tol(D) * np.maximum(1.0, np.abs(ref))).all()
        f32 = -cr.scores(tabs, h, t, r, torch.float32).astype(np.float64)
        assert (np.abs(f32 - want) <= 2 * 2.0 ** -23 * np.maximum(1.0, np.abs(want))).all()


def test_score_dev_is_measured():
    """SCORE_DEV again, from the float32 torch forward on the GPU score tests' inputs: not grown."""
    for D in cr.SCORE_DIMS:
        dev = cr.measure_score_dev(D)
        print("SCORE_DEV[%d] measured %.3e (table %.3e, tol %.3e)" % (D, dev, cr.SCORE_DEV[D], cr.score_tol(D)))
        assert dev <= cr.SCORE_DEV[D]


def test_grad_and_loss_dev_is_measured():
    """GRAD_DEV and LOSS_DEV again, from torch's float32 evaluation of every synthetic case: not grown."""
    runs = [(c[0],) + cc.build(c) for c in cc.ALL_CASES]
    for c in cc.ADAM_CASES:
        tabs, batches, cfg, _, _, _ = cc.build_adam(c)
        runs += [("%s step %d" % (c[0], s), tabs, hrt, cfg) for s, hrt in enumerate(batches)]
    for name, tabs, hrt, cfg in runs:
        g, lo = cr.measure_case_dev(tabs, hrt, cfg)
        print("%s: float32 gradient deviation %.3e, loss %.3e" % (name, g, lo))
        assert g <= cr.GRAD_DEV[cr.family(cfg)] and lo <= cr.LOSS_DEV


def _adagrad(w, acc, g, lr):
    acc = acc + g * g
    return w - lr * g / (np.sqrt(acc) + 1e-10), acc


@pytest.mark.parametrize("path", golden("complex_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_optimizer_runs_match_reference(path):
    """The reference's Adagrad (with regul_rate, bern) and Adam trajectories: float64 gradients + the Adagrad formula /
    adam_update from the recorded initial tables give its losses (rtol 1e-5), its optimizer state after step 1 and its
    final tables (the caps of test_distmult_reference_cpu.py's test of the same name)."""
    z = load(path)
    cfg = cr.golden_cfg(z)
    lr, steps, opt = float(z["lr"]), int(z["steps"]), str(z["optimizer"])
    w = [x.astype(np.float64) for x in cr.golden_tables(z, "init")]
    a = [np.zeros_like(x) for x in w]
    b = [np.zeros_like(x) for x in w]
    for s in range(steps):
        loss, grads, _ = cr.loss_and_grads(w, *cr.golden_step(z, s), cfg["batch_size"], cfg)
        assert abs(loss - float(z["losses"][s])) <= 1e-5 * abs(loss), (s, loss, float(z["losses"][s]))
        for i in range(4):
            if opt == "adam":
                w[i], a[i], b[i] = cr.adam_update(w[i], a[i], b[i], grads[i], lr, s + 1)
            else:
                w[i], a[i] = _adagrad(w[i], a[i], grads[i], lr)
        if s == 0:
            for i, k in enumerate(cr.TABLES):
                if opt == "adam":
                    np.testing.assert_allclose(a[i], z["step1_m_" + k], rtol=0, atol=1e-7)
                    np.testing.assert_allclose(b[i], z["step1_v_" + k], rtol=0, atol=1e-9)
                else:
                    np.testing.assert_allclose(a[i], z["step1_sum_" + k], rtol=0, atol=1e-9)
    cap = 2 * steps * lr * 0.1 / np.sqrt(0.001) * 1e-3 if opt == "adam" else steps * lr * 1e-3
    for got, want, name in zip(w, cr.golden_tables(z, "final"), cr.TABLES):
        dev = float(np.abs(got - want).max())
        print("%s %s: |float64 final - reference final| %.3e (cap %.3e)" % (path.split("/")[-1], name, dev, cap))
        assert dev <= cap


def lp_margins(tabs, queries):
    """[n_queries, 2]: the smallest |candidate score - truth score| / max(1, |truth score|) of every query and side, in
    float64."""
    out = np.zeros((len(queries), 2))
    for i, (h, t, r) in enumerate(queries):
        for side in (0, 1):
            row = cr.lp_scores(tabs, int(t if side == 0 else h), int(r), side)
            truth = int(h if side == 0 else t)
            d = np.abs(row - row[truth])
            d[truth] = np.inf
            out[i, side] = d.min() / max(1.0, abs(row[truth]))
    return out


def test_lp_fixture_has_no_near_ties_and_its_ranks_follow_from_float64():
    """complex_lp.npz: no candidate lies within score_tol of its query's truth score in float64, so ranks can be demanded
    exactly; and the reference's raw ranks are the float64 form's."""
    z = load(golden("complex_lp.npz")[0])
    tabs = cr.golden_tables(z, "")
    qs = z["queries"].astype(np.int64)
    margins = lp_margins(tabs, qs)
    D = int(z["dim"])
    tol = cr.score_tol(D if D in cr.SCORE_DEV else 20)
    print("complex_lp: smallest relative gap to a truth score %.3e (score_tol %.3e)" % (margins.min(), tol))
    assert margins.min() > 2 * tol   # (both scores of a comparison may move by tol)
    names = [str(n) for n in z["rank_names"]]
    for i, (h, t, r) in enumerate(qs):
        for side, key in ((0, "l_rank"), (1, "r_rank")):
            row = cr.lp_scores(tabs, int(t if side == 0 else h), int(r), side)
            truth = int(h if side == 0 else t)
            assert int((row < row[truth]).sum()) == int(z["ranks"][names.index(key)][i])
    for k in cr.TABLES:   # the recorded tables are the uniform(+-table_range) overwrite, not the construction's
        assert np.abs(z[k]).max() <= float(z["table_range"]) and not np.array_equal(z[k], z["init_" + k])


# ------------------------------------------------------------------ the Python model ------------
def test_python_complex_matches_reference_construction():
    """torch.manual_seed(s); ComplEx(...) gives the reference's four tables bit for bit, its state_dict keys and
    attributes; seeded() draws the same tables from a private generator."""
    from openke import _native
    paths = _fixtures()
    assert len(paths) == 12
    for path in paths:
        z = load(path)
        want = cr.golden_tables(z, "init")
        dim = int(z["dim"])
        E, R = want[0].shape[0], want[2].shape[0]
        torch.manual_seed(int(z["torch_seed"]))
        kge = ComplEx(ent_tot=E, rel_tot=R, dim=dim)
        torch.manual_seed(12345)   # seeded() must not read the global generator
        sd = ComplEx.seeded(int(z["torch_seed"]), E, R, dim=dim)
        for m in (kge, sd):
            for name, x in zip(cr.TABLES, want):
                np.testing.assert_array_equal(getattr(m, name).weight.detach().numpy(), x)
        assert sorted(kge.state_dict().keys()) == [str(k) for k in z["state_keys"]]
        assert {k + ".weight" for k in cr.TABLES} <= set(kge.state_dict().keys())
        assert not any(k.startswith(("ent_embeddings", "rel_embeddings")) for k in kge.state_dict())
        assert kge.dim == dim and kge.native_model == _native.PT_COMPLEX == 5 and not hasattr(kge, "margin_flag")
        ent_re, rel_re, none, ent_im, rel_im = kge.tables()
        assert none is None and ent_re is kge.ent_re_embeddings.weight and ent_im is kge.ent_im_embeddings.weight
        assert rel_re is kge.rel_re_embeddings.weight and rel_im is kge.rel_im_embeddings.weight
    assert ComplEx(3, 2).dim == 100 and not hasattr(ComplEx, "l3_regularization")


def test_reference_state_dict_loads():
    """A state_dict with exactly the reference's recorded keys (fixture tables; the two constants of BaseModule) loads
    strictly."""
    z = load(golden("complex_p2.npz")[0])
    tabs = cr.golden_tables(z, "")
    kge = ComplEx(tabs[0].shape[0], tabs[2].shape[0], dim=int(z["dim"]))
    sd = {k + ".weight": torch.from_numpy(np.array(x)) for k, x in zip(cr.TABLES, tabs)}
    sd.update({"zero_const": torch.Tensor([0]), "pi_const": torch.Tensor([3.14159265358979323846])})
    assert sorted(sd) == [str(k) for k in z["state_keys"]]
    kge.load_state_dict(sd, strict=True)
    for k, x in zip(cr.TABLES, tabs):
        np.testing.assert_array_equal(getattr(kge, k).weight.detach().numpy(), x)


def test_regularization_returns_the_reference_value():
    """regularization(data) on CPU tables against the float64 form."""
    torch.manual_seed(5)
    kge = ComplEx(9, 3, dim=6)
    rng = np.random.default_rng(1)
    h, t, r = rng.integers(0, 9, 12), rng.integers(0, 9, 12), rng.integers(0, 3, 12)
    ere, eim, rre, rim = (getattr(kge, k).weight.detach().double().numpy() for k in cr.TABLES)
    want = sum((x ** 2).mean() for x in (ere[h], eim[h], ere[t], eim[t], rre[r], rim[r])) / 6
    got = kge.regularization({"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"})
    assert abs(float(got.detach()) - want) <= 1e-6 * want
    cfg = {"loss": "sigmoid", "adv_temperature": None, "regul_rate": 1.0}
    tabs = [torch.tensor(x) for x in (ere, eim, rre, rim)]
    hh, tt, rr = (torch.as_tensor(x) for x in (h, t, r))
    with_reg, _ = cr.loss_value(tabs, hh, tt, rr, 4, cfg)
    without, _ = cr.loss_value(tabs, hh, tt, rr, 4, dict(cfg, regul_rate=0.0))
    assert abs(float(with_reg - without) - want) <= 1e-12


# ------------------------------------------------------------------ the cases' conditions -------
@pytest.mark.parametrize("case", cc.ALL_CASES, ids=lambda c: c[0])
def test_case_admission(case):
    tabs, hrt, cfg = cc.build(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    assert all(cc.planted(*hrt, bs, K, "normal").values())
    fig = cc.admission(tabs, hrt, cfg)
    bound, dev32, (lo, hi), effect, wrong = fig
    print("%s: bound %.3e, torch float32 dev %.3e, scores [%.2f, %.2f], regulariser effect %s, sign flip %s, im zeroed %s"
          % (case[0], bound, dev32, lo, hi, effect, wrong["flip"], wrong["no_im"]))
    assert dev32 <= bound / 4
    assert lo <= -2 and hi >= 2
    if cfg["regul_rate"]:
        assert effect > 20 * bound
    for variant, moved in wrong.items():
        assert len(moved) == 4 and all(x > 20 * bound for x in moved), (variant, moved, bound)
    if case[0] == cc.THRESHOLD_CASE[0]:
        assert hi > 20
    if case[0] == cc.MANY_REL_CASE[0]:
        h, t, r = (x[bs:].reshape(K, bs) for x in hrt)
        assert int((r[:, 2] != hrt[2][2]).sum()) >= cc.MANY_REL > 4
        assert h[0, 5] != hrt[0][5] and t[0, 5] != hrt[1][5]


@pytest.mark.parametrize("case", cc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_case_admission(case):
    tabs, batches, cfg, (m0, v0), lr, step0 = cc.build_adam(case)
    for s, hrt in enumerate(batches):
        assert cc.FREE_ENT not in hrt[0] and cc.FREE_ENT not in hrt[1] and cc.FREE_REL not in hrt[2]
        assert ((cc.ONCE_ENT in hrt[0]) or (cc.ONCE_ENT in hrt[1])) == (s == 0)
        assert cc.admitted(cc.admission(tabs, hrt, cfg), cfg)
    for m, v in zip(m0, v0):
        row = cc.FREE_REL if m.shape[0] == cr.R else cc.FREE_ENT
        assert not m[row].any() and not v[row].any() and m[0].any() and v[0].any()


def test_case_shapes_cover_the_issue():
    dims = {c[1] for c in cc.GRAD_CASES}
    assert dims == {1, 2, 3, 5, 8, 20, 200, 260, 512, 516, 1024}
    assert {c[2] for c in cc.GRAD_CASES} == {11, 37} and {1, 3, 7} <= {c[3] for c in cc.GRAD_CASES}
    assert {(c[1], c[3]) for c in cc.GRAD_CASES} >= {(8, 70), (20, 70), (1024, 130)}


# ------------------------------------------------------------------ refusals without a device ---
def _ns(kge, loss, **kw):
    from openke.module.strategy import NegativeSampling
    return NegativeSampling(model=kge, loss=loss, batch_size=2, **kw)


class _Loader(object):
    def __init__(self, sampling_mode):
        self.sampling_mode = sampling_mode


def test_trainer_parts_accepts_and_refuses_by_name():
    """Trainer._parts (no device): ComplEx passes with SigmoidLoss / SoftplusLoss, with or without the temperature and
    regul_rate; MarginLoss, l3_regul_rate, a loader that does not sample in normal mode and deterministic=True are
    refused with a message that names ComplEx."""
    from openke.config import Trainer
    torch.manual_seed(1)
    kge = ComplEx(6, 2, dim=8)
    for loss in (SigmoidLoss(), SigmoidLoss(adv_temperature=1.0), SoftplusLoss(), SoftplusLoss(adv_temperature=0.5)):
        for kw in ({}, {"regul_rate": 1.0}):
            for dl in (None, _Loader("normal")):
                ns, got, lo = Trainer(model=_ns(kge, loss, **kw), data_loader=dl)._parts()
                assert got is kge and lo is loss
    with pytest.raises(NotImplementedError, match="MarginLoss on ComplEx"):
        Trainer(model=_ns(kge, MarginLoss(margin=1.0)), data_loader=None)._parts()
    with pytest.raises(NotImplementedError, match="l3_regul_rate on ComplEx"):
        Trainer(model=_ns(kge, SoftplusLoss(), l3_regul_rate=1e-3), data_loader=None)._parts()
    with pytest.raises(NotImplementedError, match="ComplEx trains on normal sampling only"):
        Trainer(model=_ns(kge, SoftplusLoss()), data_loader=_Loader("cross"))._parts()
    with pytest.raises(NotImplementedError, match="not implemented for ComplEx"):
        Trainer(model=_ns(kge, SoftplusLoss()), data_loader=None, deterministic=True)._parts()


def test_universe_configuration_refuses_complex():
    from openke.config import Parallel_Universe_Config
    pu = object.__new__(Parallel_Universe_Config)
    pu.embedding_model = ComplEx
    with pytest.raises(NotImplementedError, match="ComplEx"):
        pu._check_setup()


def test_native_constants_and_dim_rule():
    from openke import _native
    assert _native.PT_COMPLEX == 5
    L = _native.lib()
    for dim in (1, 200, 512, 516, 1024, 1028):
        assert L.pt_model_dim_supported(dim, _native.PT_COMPLEX) == 0
    assert L.pt_version() == 1
