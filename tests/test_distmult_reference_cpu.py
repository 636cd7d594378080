"""distmult_reference.py (the float64 form of DistMult with both regularisers) against the reference implementation's
own float32 runs (tests/golden/distmult_*.npz, written by tests/golden/make_golden_distmult.py), the Python DistMult
and SoftplusLoss, the Python-side refusals that need no device, and the input conditions of the GPU cases of
test_gpu_distmult.py checked on the CPU."""
import numpy as np
import pytest
import torch

import distmult_cases as dc
import distmult_reference as dr
from helpers import golden, load
from openke.module.loss import SigmoidLoss, SoftplusLoss
from openke.module.model import DistMult   # (no test of this file means anything without the model)

TIE_REL = 4e-6   # test_gpu_realscale.py's near-tie band, relative to max(1, |truth score|)


def _margin(z):
    g, e = float(z["model_margin"]), float(z["epsilon"])
    return (None, None) if np.isnan(g) else (g, e)


@pytest.mark.parametrize("path", golden("distmult_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_gradients_match_reference_runs(path):
    """Every SGD lr 1 step of the reference: its table delta is the float64 gradient at the tables before it within
    GRAD_DEV of the case's family, its loss the float64 loss within LOSS_DEV (both measured again: not grown)."""
    z = load(path)
    cfg = dr.golden_cfg(z)
    fam = dr.family(cfg)
    assert int(z["steps"]) >= 2 and float(z["lr"]) == 1.0
    dev, ldev = dr.measure_grad_dev(z)
    print("%s: family %s GRAD_DEV measured %.3e (table %.3e), LOSS_DEV measured %.3e (table %.3e)"
          % (path.split("/")[-1], fam, dev, dr.GRAD_DEV[fam], ldev, dr.LOSS_DEV))
    assert dev <= dr.GRAD_DEV[fam], (fam, dev)
    assert ldev <= dr.LOSS_DEV, ldev


def test_golden_cases_cover_the_issue():
    """SigmoidLoss and SoftplusLoss, each with and without the temperature, normal and cross sampling, regul_rate 0
    and 1, dims 5, 7, 8, 12, 16, 20; both init branches."""
    seen = set()
    dims, regs, inits = set(), set(), set()
    for path in golden("distmult_g*.npz"):
        cfg = dr.golden_cfg(load(path))
        seen.add((cfg["loss"], cfg["adv_temperature"] is not None))
        seen.add((cfg["loss"], cfg["sampling"]))
        dims.add(cfg["dim"])
        regs.add(cfg["regul_rate"])
        inits.add(cfg["model_margin"] is None)
    assert {dr.family(dr.golden_cfg(load(p))) for p in golden("distmult_g*.npz")} == set(dr.GRAD_DEV)
    for lo in ("sigmoid", "softplus"):
        assert {(lo, True), (lo, False), (lo, "normal"), (lo, "cross")} <= seen
    assert dims == {5, 7, 8, 12, 16, 20} and regs == {0.0, 1.0} and inits == {True, False}


@pytest.mark.parametrize("path", golden("distmult_p*.npz"), ids=lambda p: p.split("/")[-1])
def test_predict_matches_reference(path):
    """The reference's predict (-s) in the three modes: the float64 scores to float32 rounding, and the float32
    evaluation of the same forward (what SCORE_DEV measures) to two ulps."""
    z = load(path)
    tabs = dr.golden_tables(z, "")
    for mode in ("normal", "head_batch", "tail_batch"):
        h, t, r = dr.expand_predict(z[mode + "_h"], z[mode + "_t"], z[mode + "_r"], mode)
        want = z[mode + "_score"].astype(np.float64)
        ref = -dr.scores(tabs, h, t, r, mode)
        got32 = -dr.scores(tabs, h, t, r, mode, torch.float32).astype(np.float64)
        scale = np.maximum(1.0, np.abs(ref))
        assert (np.abs(want - ref) / scale).max() <= 1e-6
        assert (np.abs(want - got32) / scale).max() <= 2 * 2.0 ** -23


def test_score_dev_is_measured():
    """SCORE_DEV again, from the float32 torch forward on the GPU score tests' inputs: not grown."""
    for D in dr.SCORE_DIMS:
        dev = dr.measure_score_dev(D)
        print("SCORE_DEV[%d] measured %.3e (table %.3e, tol %.3e)" % (D, dev, dr.SCORE_DEV[D], dr.score_tol(D)))
        assert dev <= dr.SCORE_DEV[D]


@pytest.mark.parametrize("path", golden("distmult_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_optimizer_runs_match_reference(path):
    """The reference's Adam (with l3_regul_rate) and Adagrad (with regul_rate) trajectories: float64 gradients +
    adam_update / the Adagrad formula from the recorded initial tables give its losses and its final tables (the caps
    of test_rotate_reference_cpu.py's test of the same name) and its optimizer state after step 1."""
    z = load(path)
    cfg = dr.golden_cfg(z)
    lr, steps, opt = float(z["lr"]), int(z["steps"]), str(z["optimizer"])
    assert (cfg["l3_regul_rate"] > 0) == (opt == "adam") and (cfg["regul_rate"] > 0) == (opt == "adagrad")
    w = [x.astype(np.float64) for x in dr.golden_tables(z, "init")]
    m = [np.zeros_like(x) for x in w]
    v = [np.zeros_like(x) for x in w]
    for s in range(steps):
        (h, t, r), mode = dr.golden_step(z, cfg, s)
        loss, grads, _ = dr.loss_and_grads(w, h, t, r, cfg["batch_size"], cfg, mode)
        np.testing.assert_allclose(loss, float(z["losses"][s]), rtol=1e-4)
        for i in range(2):
            if opt == "adam":
                w[i], m[i], v[i] = dr.adam_update(w[i], m[i], v[i], grads[i], lr, s + 1)
            else:
                v[i] = v[i] + grads[i] * grads[i]
                w[i] = w[i] - lr * grads[i] / (np.sqrt(v[i]) + 1e-10)
        if s == 0:
            for i, nm in enumerate(dr.TABLES):
                if opt == "adam":
                    np.testing.assert_allclose(m[i], z["step1_m_" + nm], rtol=0, atol=1e-7)
                    np.testing.assert_allclose(v[i], z["step1_v_" + nm], rtol=1e-4, atol=1e-12)
                else:
                    np.testing.assert_allclose(v[i], z["step1_sum_" + nm], rtol=1e-4, atol=1e-12)
    cap = 2 * steps * lr * (1 - 0.9) / np.sqrt(1 - 0.999) if opt == "adam" else steps * lr * 1e-3
    for i, nm in enumerate(dr.TABLES):
        assert np.abs(w[i] - z["final_" + nm]).max() <= cap


def test_python_distmult_matches_reference_construction():
    """torch.manual_seed(s); DistMult(...) gives the reference's tables bit for bit in both init branches, its
    state_dict keys and attributes; seeded() draws the same tables from a private generator."""
    from openke import _native
    paths = (golden("distmult_g*.npz") + golden("distmult_a*.npz") + golden("distmult_p*.npz") +
             golden("distmult_lp.npz"))
    assert len(paths) == 12
    branches = set()
    for path in paths:
        z = load(path)
        want = dr.golden_tables(z, "init")
        dim = int(z["dim"])
        gamma, eps = _margin(z)
        branches.add(gamma is None)
        torch.manual_seed(int(z["torch_seed"]))
        kge = DistMult(ent_tot=want[0].shape[0], rel_tot=want[1].shape[0], dim=dim, margin=gamma, epsilon=eps)
        np.testing.assert_array_equal(kge.ent_embeddings.weight.detach().numpy(), want[0])
        np.testing.assert_array_equal(kge.rel_embeddings.weight.detach().numpy(), want[1])
        assert sorted(kge.state_dict().keys()) == [str(k) for k in z["state_keys"]]
        assert kge.dim == dim and kge.margin == gamma and kge.epsilon == eps
        assert hasattr(kge, "embedding_range") == (gamma is not None)
        if gamma is not None:
            assert kge.embedding_range.item() == torch.Tensor([(gamma + eps) / dim]).item()
            assert not kge.embedding_range.requires_grad
        assert kge.native_model == _native.PT_DISTMULT == 4 and not hasattr(kge, "margin_flag")
        torch.manual_seed(12345)   # seeded() must not read the global generator
        sd = DistMult.seeded(int(z["torch_seed"]), want[0].shape[0], want[1].shape[0], dim=dim, margin=gamma,
                             epsilon=eps)
        np.testing.assert_array_equal(sd.ent_embeddings.weight.detach().numpy(), want[0])
        np.testing.assert_array_equal(sd.rel_embeddings.weight.detach().numpy(), want[1])
    assert branches == {True, False}


def test_regularization_methods_return_the_reference_values():
    """regularization(data) and l3_regularization() on CPU tables against the float64 form."""
    torch.manual_seed(5)
    kge = DistMult(9, 3, dim=6)
    rng = np.random.default_rng(1)
    h, t, r = rng.integers(0, 9, 12), rng.integers(0, 9, 12), rng.integers(0, 3, 12)
    ent = kge.ent_embeddings.weight.detach().double().numpy()
    rel = kge.rel_embeddings.weight.detach().double().numpy()
    want = ((ent[h] ** 2).mean() + (ent[t] ** 2).mean() + (rel[r] ** 2).mean()) / 3
    got = kge.regularization({"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"})
    assert abs(float(got.detach()) - want) <= 1e-6 * want
    # tail_batch as the loader hands it over: h and r once per positive
    got = kge.regularization({"batch_h": h[:4], "batch_t": t, "batch_r": r[:4], "mode": "tail_batch"})
    want = ((ent[h[:4]] ** 2).mean() + (ent[t] ** 2).mean() + (rel[r[:4]] ** 2).mean()) / 3
    assert abs(float(got.detach()) - want) <= 1e-6 * want
    want = (np.abs(ent) ** 3).sum() + (np.abs(rel) ** 3).sum()
    assert abs(float(kge.l3_regularization().detach()) - want) <= 1e-5 * want


def test_softplus_loss_class():
    """The reference's class: attributes, weights, and values equal to SigmoidLoss's to float32 (and exactly the
    threshold form beyond 20)."""
    rng = np.random.default_rng(3)
    p = torch.from_numpy(rng.normal(0, 3, size=(7, 1)).astype(np.float32))
    n = torch.from_numpy(rng.normal(0, 3, size=(7, 5)).astype(np.float32))
    n[0, 0], p[1, 0] = 25.0, -30.0   # beyond the threshold
    for temp in (None, 0.5):
        sp, sg = SoftplusLoss(adv_temperature=temp), SigmoidLoss(adv_temperature=temp)
        assert sp.adv_flag == (temp is not None) and isinstance(sp.criterion, torch.nn.Softplus)
        if temp is not None:
            assert sp.adv_temperature.item() == temp and not sp.adv_temperature.requires_grad
            np.testing.assert_array_equal(sp.get_weights(n).numpy(), torch.softmax(n * temp, -1).numpy())
        a, b = float(sp(p, n)), float(sg(p, n))
        assert abs(a - b) <= 4 * 2.0 ** -23 * max(1.0, abs(b)), (a, b)
        assert sp.predict(p, n) == sp(p, n).numpy()
        pd, nd = p.double(), n.double()
        w = torch.softmax(nd * temp, -1) if temp is not None else torch.full_like(nd, 1.0 / nd.shape[1])
        f = torch.nn.functional.softplus
        want = float((f(-pd).mean() + (w * f(nd)).sum(-1).mean()) / 2)
        assert abs(a - want) <= 4 * 2.0 ** -23 * max(1.0, abs(want))
    assert set(sp.state_dict().keys()) == set(sg.state_dict().keys()) >= {"adv_temperature"}


def test_softplus_threshold_form_is_sigmoid_loss_to_float32():
    """The issue's argument, checked on the threshold case in float64: the threshold form and the logsigmoid form give
    the same loss and gradients far inside the cell bound."""
    tabs, hrt, cfg, mode = dc.build(dc.THRESHOLD_CASE)
    bs = cfg["batch_size"]
    la, ga, aux = dr.loss_and_grads(tabs, *hrt, bs, cfg, mode)
    lb, gb, _ = dr.loss_and_grads(tabs, *hrt, bs, dict(cfg, loss="sigmoid"), mode)
    assert np.abs(aux["s"]).max() > 20
    assert abs(la - lb) <= 1e-8
    assert max(float(np.abs(a - b).max()) for a, b in zip(ga, gb)) <= 1e-8


# ------------------------------------------------------------------ the GPU cases' input conditions
@pytest.mark.parametrize("case", dc.ALL_CASES, ids=lambda c: c[0])
def test_case_admission(case):
    tabs, hrt, cfg, mode = dc.build(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    flags = dc.planted(*hrt, bs, K, mode)
    assert all(v for k, v in flags.items() if k != "other_relation") and flags["other_relation"] == (mode == "normal")
    bound, dev32, (lo, hi), effect = dc.admission(tabs, hrt, cfg, mode)
    print("%s: bound %.3e, torch float32 dev %.3e, scores [%.2f, %.2f], regulariser effect %s"
          % (case[0], bound, dev32, lo, hi, effect))
    assert dev32 <= bound / 4
    assert lo <= -2 and hi >= 2
    if cfg["regul_rate"]:
        assert effect > 20 * bound
    if case[0] == dc.THRESHOLD_CASE[0]:
        assert max(-lo, hi) > 20


@pytest.mark.parametrize("case", dc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_case_admission(case):
    tabs, batches, cfg, (m0, v0), lr, step0 = dc.build_adam(case)
    for hrt in batches:
        assert dc.FREE_ENT not in hrt[0] and dc.FREE_ENT not in hrt[1] and dc.FREE_REL not in hrt[2]
        bound, dev32, (lo, hi), effect = dc.admission(tabs, hrt, cfg, "normal")
        assert dev32 <= bound / 4 and lo <= -2 and hi >= 2
        if cfg["l3_regul_rate"] or cfg["regul_rate"]:
            assert effect > 20 * bound
    if cfg["l3_regul_rate"]:
        # L3 alone moves the never-drawn rows by far more than a bound
        g = 3 * cfg["l3_regul_rate"] * np.abs(tabs[0][dc.FREE_ENT].astype(np.float64)) ** 2
        assert g.max() > 20 * dr.grad_bound(dr.family(cfg), 1.0)
    assert not m0[0][dc.FREE_ENT].any() and not v0[0][dc.FREE_ENT].any()
    assert not m0[1][dc.FREE_REL].any() and not v0[1][dc.FREE_REL].any()


# ------------------------------------------------------------------ refusals that need no device
def _ns(kge, loss, **kw):
    from openke.module.strategy import NegativeSampling
    return NegativeSampling(model=kge, loss=loss, batch_size=2, **kw)


def test_trainer_parts_accepts_and_refuses_by_name():
    """Trainer._parts (no device): DistMult passes with SigmoidLoss / SoftplusLoss and both regularisers; MarginLoss on
    DistMult, SoftplusLoss or a regulariser on any other model are refused by name."""
    from openke.config import Trainer
    from openke.module.loss import MarginLoss
    from openke.module.model import RotatE, TransE
    torch.manual_seed(1)
    dm = DistMult(6, 2, dim=8)
    for loss, kw in ((SigmoidLoss(adv_temperature=0.5), {"l3_regul_rate": 5e-6}), (SoftplusLoss(), {"regul_rate": 1.0}),
                     (SoftplusLoss(adv_temperature=1.0), {})):
        ns, kge, lo = Trainer(model=_ns(dm, loss, **kw), data_loader=None)._parts()
        assert kge is dm and lo is loss
        assert Trainer._weighted(kge, lo)
    with pytest.raises(NotImplementedError, match="MarginLoss on DistMult"):
        Trainer(model=_ns(dm, MarginLoss(margin=1.0)), data_loader=None)._parts()
    for other in (TransE(6, 2, dim=8), RotatE(6, 2, dim=8)):
        with pytest.raises(NotImplementedError, match="SoftplusLoss"):
            Trainer(model=_ns(other, SoftplusLoss()), data_loader=None)._parts()
        for kw in ({"regul_rate": 0.1}, {"l3_regul_rate": 0.1}):
            with pytest.raises(NotImplementedError, match="regularisation"):
                Trainer(model=_ns(other, SigmoidLoss(), **kw), data_loader=None)._parts()


def test_universe_configuration_refuses_distmult():
    from openke.config import Parallel_Universe_Config
    pu = object.__new__(Parallel_Universe_Config)
    pu.embedding_model = DistMult
    with pytest.raises(NotImplementedError, match="DistMult"):
        pu._check_setup()


def test_native_constants():
    from openke import _native
    assert _native.PT_DISTMULT == 4
    rd = _native.RegulDesc()
    assert [f[0] for f in rd._fields_] == ["regul_rate", "l3_regul_rate", "batch_mode"]
    assert hasattr(_native.lib(), "pt_trainer_set_regul")
    L = _native.lib()
    # the query keeps answering for models 0-2 only; universes do not take the model
    assert L.pt_model_dim_supported(20, _native.PT_DISTMULT) == 0
    assert L.pt_universe_dim_supported(20, _native.PT_DISTMULT) == 0


# ------------------------------------------------------------------ link prediction near-ties
def lp_excused(tabs, queries):
    """[n_queries, 2] bool: whether a query's float64 score vector (side 0 head, 1 tail prediction) holds a candidate
    within TIE_REL of the truth's score (relative to max(1, |truth score|)): such a rank may differ by float32
    rounding between two correct implementations."""
    out = np.zeros((len(queries), 2), dtype=bool)
    for i, (h, t, r) in enumerate(queries):
        for side in (0, 1):
            row = dr.lp_scores(tabs, int(t if side == 0 else h), int(r), side)
            truth = int(h if side == 0 else t)
            d = np.abs(row - row[truth])
            d[truth] = np.inf
            out[i, side] = d.min() <= TIE_REL * max(1.0, abs(row[truth]))
    return out


def test_reference_ranks_follow_from_the_float64_scores():
    """distmult_lp.npz: outside near-ties the reference's raw ranks are the float64 form's."""
    z = load(golden("distmult_lp.npz")[0])
    tabs = dr.golden_tables(z, "")
    qs = z["queries"].astype(np.int64)
    excused = lp_excused(tabs, qs)
    assert excused.mean() <= 0.02
    names = [str(x) for x in z["rank_names"]]
    for side, nm in ((0, "l_rank"), (1, "r_rank")):
        want = z["ranks"][names.index(nm)].astype(np.int64)
        for i, (h, t, r) in enumerate(qs):
            if excused[i, side]:
                continue
            row = dr.lp_scores(tabs, int(t if side == 0 else h), int(r), side)
            truth = int(h if side == 0 else t)
            assert int((row < row[truth]).sum()) == want[i], (nm, i)
