"""rotate_reference.py (the float64 form of RotatE) against the reference implementation's own float32 runs
(tests/golden/rotate_*.npz, written by tests/golden/make_golden_rotate.py), the Python RotatE's construction, the
Python-side refusals that need no device, and the input conditions of the GPU cases of test_gpu_rotate.py checked on
the CPU."""
import numpy as np
import pytest
import torch

import rotate_cases as rc
import rotate_reference as rr
from helpers import golden, load
from openke.module.model import RotatE   # (no test of this file means anything without the model)

TIE_REL = 4e-6   # test_gpu_realscale.py's near-tie band, relative to max(1, |truth score|)


@pytest.mark.parametrize("path", golden("rotate_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_gradients_match_reference_runs(path):
    """Every SGD lr 1 step of the reference: its table delta is the float64 gradient at the tables before it within
    4 GRAD_DEV of the case's family (and within GRAD_DEV, which this measures again: not grown), its loss the float64
    loss."""
    z = load(path)
    cfg = rr.golden_cfg(z)
    fam = rr.family(cfg)
    assert int(z["steps"]) >= 2 and float(z["lr"]) == 1.0
    for s in range(int(z["steps"])):
        before = rr.golden_tables(z, "s%d" % s)
        (h, t, r), mode = rr.golden_step(z, cfg, s)
        loss, _, aux = rr.loss_and_grads(before, h, t, r, cfg["batch_size"], cfg, mode)
        np.testing.assert_allclose(loss, float(z["losses"][s]), rtol=1e-6)
    dev = rr.measure_grad_dev(z)
    print("%s: family %s GRAD_DEV measured %.3e (table %.3e)" % (path.split("/")[-1], fam, dev, rr.GRAD_DEV[fam]))
    assert dev <= rr.GRAD_DEV[fam], (fam, dev)


def test_grad_dev_table_covers_every_family():
    """Every family of the table is measured by a golden case: SigmoidLoss and MarginLoss, each with and without the
    adversarial weights, normal and cross sampling, an odd dim and a multiple of 4."""
    seen, samplings, dims = set(), set(), set()
    for path in golden("rotate_g*.npz"):
        cfg = rr.golden_cfg(load(path))
        seen.add(rr.family(cfg))
        samplings.add((cfg["loss"], cfg["sampling"]))
        dims.add(cfg["dim"])
    assert seen == set(rr.GRAD_DEV)
    assert samplings == {(lo, sa) for lo in ("sigmoid", "margin") for sa in ("normal", "cross")}
    assert any(d % 2 for d in dims) and any(d % 4 == 0 for d in dims)


@pytest.mark.parametrize("path", golden("rotate_p*.npz"), ids=lambda p: p.split("/")[-1])
def test_predict_matches_reference(path):
    """The reference's predict (distance - margin) in the three modes: the float64 distances to float32 rounding, and
    the float32 evaluation of the same forward (what SCORE_DEV measures) to two ulps of the distance."""
    z = load(path)
    tabs = rr.golden_tables(z, "")
    q, gamma = rr.phase_div(float(z["rel_embedding_range"])), float(z["model_margin"])
    for mode in ("normal", "head_batch", "tail_batch"):
        h, t, r = rr.expand_predict(z[mode + "_h"], z[mode + "_t"], z[mode + "_r"], mode)
        want = z[mode + "_score"].astype(np.float64) + gamma
        ref = rr.scores(tabs, h, t, r, q, mode)
        got32 = rr.scores(tabs, h, t, r, q, mode, torch.float32).astype(np.float64)
        scale = np.maximum(1.0, ref)
        assert (np.abs(want - ref) / scale).max() <= 1e-6
        assert (np.abs(want - got32) / scale).max() <= 2 * 2.0 ** -23


def test_score_dev_is_measured():
    """SCORE_DEV again, from the float32 torch forward on the GPU score tests' inputs: not grown."""
    for D in rr.SCORE_DIMS:
        dev = rr.measure_score_dev(D)
        print("SCORE_DEV[%d] measured %.3e (table %.3e, tol %.3e)" % (D, dev, rr.SCORE_DEV[D], rr.score_tol(D)))
        assert dev <= rr.SCORE_DEV[D]


@pytest.mark.parametrize("path", golden("rotate_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_optimizer_runs_match_reference(path):
    """The reference's Adam and Adagrad trajectories: float64 gradients + adam_update / the Adagrad formula from the
    recorded initial tables give its losses and its final tables (the caps of test_transd_reference_cpu.py's test of
    the same name) and its optimizer state after step 1."""
    z = load(path)
    cfg = rr.golden_cfg(z)
    lr, steps, opt = float(z["lr"]), int(z["steps"]), str(z["optimizer"])
    w = [x.astype(np.float64) for x in rr.golden_tables(z, "init")]
    m = [np.zeros_like(x) for x in w]
    v = [np.zeros_like(x) for x in w]
    for s in range(steps):
        (h, t, r), mode = rr.golden_step(z, cfg, s)
        loss, grads, _ = rr.loss_and_grads(w, h, t, r, cfg["batch_size"], cfg, mode)
        np.testing.assert_allclose(loss, float(z["losses"][s]), rtol=1e-4)
        for i in range(2):
            if opt == "adam":
                w[i], m[i], v[i] = rr.adam_update(w[i], m[i], v[i], grads[i], lr, s + 1)
            else:
                v[i] = v[i] + grads[i] * grads[i]
                w[i] = w[i] - lr * grads[i] / (np.sqrt(v[i]) + 1e-10)
        if s == 0:
            for i, nm in enumerate(rr.TABLES):
                if opt == "adam":
                    np.testing.assert_allclose(m[i], z["step1_m_" + nm], rtol=0, atol=1e-7)
                    np.testing.assert_allclose(v[i], z["step1_v_" + nm], rtol=1e-4, atol=1e-12)
                else:
                    np.testing.assert_allclose(v[i], z["step1_sum_" + nm], rtol=1e-4, atol=1e-12)
    cap = 2 * steps * lr * (1 - 0.9) / np.sqrt(1 - 0.999) if opt == "adam" else steps * lr * 1e-3
    for i, nm in enumerate(rr.TABLES):
        assert np.abs(w[i] - z["final_" + nm]).max() <= cap


def test_python_rotate_matches_reference_construction():
    """torch.manual_seed(s); RotatE(...) gives the reference's tables bit for bit, its state_dict keys, attributes and
    phase divisor; seeded() draws the same tables from a private generator."""
    from openke import _native
    paths = golden("rotate_g*.npz") + golden("rotate_a*.npz") + golden("rotate_p*.npz") + golden("rotate_lp.npz")
    assert len(paths) == 14
    for path in paths:
        z = load(path)
        want = rr.golden_tables(z, "init")
        dim, gamma, eps = int(z["dim"]), float(z["model_margin"]), float(z["epsilon"])
        assert want[0].shape[1] == 2 * dim and want[1].shape[1] == dim
        torch.manual_seed(int(z["torch_seed"]))
        kge = RotatE(ent_tot=want[0].shape[0], rel_tot=want[1].shape[0], dim=dim, margin=gamma, epsilon=eps)
        for name, w in zip(rr.TABLES, want):
            np.testing.assert_array_equal(getattr(kge, name).weight.detach().numpy(), w, err_msg=path)
        assert sorted(kge.state_dict().keys()) == [str(k) for k in z["state_keys"]]
        assert (kge.dim_e, kge.dim_r, kge.epsilon) == (2 * dim, dim, eps) and kge.margin.item() == gamma
        assert not kge.margin.requires_grad and kge.margin_flag
        assert kge.rel_embedding_range.item() == float(z["rel_embedding_range"])
        assert kge.phase_divisor() == rr.phase_div(float(z["rel_embedding_range"]))
        assert [t is None for t in kge.tables()] == [False, False, True]
    assert RotatE.native_model == _native.PT_ROTATE == 3
    z = load(golden("rotate_g1.npz")[0])
    seeded = RotatE.seeded(int(z["torch_seed"]), 5, 2, dim=8)
    torch.manual_seed(int(z["torch_seed"]))
    plain = RotatE(5, 2, dim=8)
    for a, b in zip(seeded.tables(), plain.tables()):
        assert a is None or torch.equal(a, b)
    with pytest.raises(NotImplementedError, match="regularisation"):
        plain.regularization({})


def test_python_refusals_that_need_no_device():
    """Parallel_Universe_Config names RotatE; the Trainer refuses regularisation, lr_decay and weight_decay with it
    before it touches a device; native_desc refuses CPU tables."""
    from openke.config import Parallel_Universe_Config, Trainer
    from openke.module.loss import SigmoidLoss
    from openke.module.strategy import NegativeSampling
    pu = object.__new__(Parallel_Universe_Config)
    pu.embedding_model = RotatE
    with pytest.raises(NotImplementedError, match="RotatE"):
        pu._check_setup()
    kge = RotatE(6, 2, dim=4)
    for kw in ({"regul_rate": 0.1}, {"l3_regul_rate": 0.1}):
        ns = NegativeSampling(model=kge, loss=SigmoidLoss(adv_temperature=2), batch_size=2, **kw)
        with pytest.raises(NotImplementedError, match="regularisation"):
            Trainer(model=ns, data_loader=None, train_times=0, alpha=0.1, use_gpu=True)._parts()
    ns = NegativeSampling(model=kge, loss=SigmoidLoss(adv_temperature=2), batch_size=2)
    trn = Trainer(model=ns, data_loader=None, train_times=0, alpha=0.1, use_gpu=True)
    assert trn._parts()[1] is kge and trn._weighted(kge, ns.loss)
    trn.set_lr_decay(0.1)
    with pytest.raises(NotImplementedError, match="lr_decay"):
        trn._parts()
    with pytest.raises(RuntimeError, match="cuda"):
        kge.native_desc()


def lp_excused(tabs, q, phase_div):
    """[2][n] whether query n's side holds a candidate other than the truth within TIE_REL of the truth's distance."""
    out = np.zeros((2, len(q)), dtype=bool)
    for i, (h, t, r) in enumerate(q):
        for side, truth, anchor in ((0, h, t), (1, t, h)):
            s = rr.lp_scores(tabs, int(anchor), int(r), side, phase_div)
            near = np.abs(s - s[truth]) <= TIE_REL * max(1.0, abs(s[truth]))
            out[side, i] = near.sum() > 1
    return out


def test_lp_fixture_near_ties_are_rare():
    """rotate_lp.npz: at most 2 % of the queries hold a candidate within TIE_REL of the truth's float64 distance (the
    queries test_gpu_rotate.py may excuse from rank equality)."""
    z = load(golden("rotate_lp.npz")[0])
    tabs = rr.golden_tables(z, "")
    q = z["queries"].astype(np.int64)
    excused = lp_excused(tabs, q, rr.phase_div(float(z["rel_embedding_range"])))
    print("rotate_lp: %d of %d (query, side) pairs hold a near tie" % (int(excused.sum()), excused.size))
    assert excused.any(axis=0).mean() <= 0.02


@pytest.mark.parametrize("case", rc.ALL_CASES, ids=lambda c: c[0])
def test_gpu_case_input_conditions(case):
    """The seeds, scales, margins and planted slots of the GPU cases, in float64: the batch well formed, every planted
    slot present, the distances straddling gamma, 20-80 % of a MarginLoss case's pairs active and no hinge argument
    within 1e-5 of the kink, four times the worst conditioning estimate of any gradient cell within the cell's bound,
    torch's own float32 gradients within a quarter of it."""
    tabs, (h, t, r), cfg, mode = rc.build(case)
    bs, K, D = cfg["batch_size"], cfg["neg_ent"], cfg["dim"]
    assert h.size == t.size == r.size == bs * (K + 1)
    assert h.min() >= 0 and t.min() >= 0 and max(h.max(), t.max()) < rr.E and 0 <= r.min() and r.max() < rr.R
    b = rc.as_batch((h, t, r), bs, mode)
    for x, y in zip(rr.expand_batch(b["batch_h"], b["batch_t"], b["batch_r"], mode, bs), (h, t, r)):
        np.testing.assert_array_equal(x, y)   # the mode's compact form holds the same slots
    flags = rc.planted(h, t, r, bs, K, mode)
    assert all(v for k, v in flags.items() if k != "other_relation"), flags
    assert flags["other_relation"] == (mode == "normal")
    er, rel_r = rr.init_ranges(D, rc.GAMMA, rc.EPS)
    assert np.abs(tabs[0]).max() <= case[8] * er and np.abs(tabs[1]).max() <= rel_r
    assert np.abs(tabs[1].astype(np.float64) / cfg["phase_div"]).max() <= np.pi * (1 + 1e-6)
    bound, cond, dev32, active, (dmin, dmax) = rc.admission(tabs, (h, t, r), cfg, mode)
    print("%s: bound %.3e, 4 x conditioning %.3e, torch float32 deviation %.3e, active %.2f, d in [%.3f, %.3f]"
          % (case[0], bound, cond, dev32, active, dmin, dmax))
    assert dmin < rc.GAMMA < dmax
    if cfg["loss"] == "margin":
        assert 0.2 <= active <= 0.8
        _, _, aux = rr.loss_and_grads(tabs, h, t, r, bs, cfg, mode)
        assert aux["hinge_gap"] >= 1e-5
    assert cond <= bound, (cond, bound)
    assert dev32 <= bound / 4, (dev32, bound)


def test_gpu_cases_cover_the_issue():
    """One case per dim of the issue's list, both batch sizes, K in {1, 3, 7} and two K > 64, all four loss forms,
    all three batch modes."""
    dims = [c[1] for c in rc.GRAD_CASES]
    assert sorted(set(dims)) == [1, 2, 3, 5, 8, 20, 200, 260, 512, 516, 1024]
    assert {c[2] for c in rc.GRAD_CASES} == {11, 37}
    assert {c[3] for c in rc.GRAD_CASES} == {1, 3, 7, 70, 130}
    assert {(c[1], c[3]) for c in rc.GRAD_CASES if c[3] > 64} == {(8, 70), (1024, 130)}
    assert {rr.family(rc.case_cfg(c)) for c in rc.GRAD_CASES} == set(rr.GRAD_DEV)
    assert {c[4] for c in rc.GRAD_CASES} == {"normal", "head_batch", "tail_batch"}
    for c in rc.GRAD_CASES:
        if c[3] > 64:
            assert c[6] is not None   # the strided softmax loops run under the adversarial weights


@pytest.mark.parametrize("case", rc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_case_input_conditions(case):
    tabs, batches, cfg, (m0, v0), lr, step0 = rc.build_adam(case)
    for s, (h, t, r) in enumerate(batches):
        used = set(h.tolist()) | set(t.tolist())
        assert rc.FREE_ENT not in used and (rc.ONCE_ENT in used) == (s == 0)
    assert not m0[0][rc.ONCE_ENT:].any() and not v0[0][rc.ONCE_ENT:].any() and m0[0][:rc.ONCE_ENT].any()
