"""transd_reference.py (the float64 form of TransD) against the reference implementation's own float32 runs
(tests/golden/transd_*.npz, written by tests/golden/make_golden_transd.py), the Python TransD's construction, and the
input conditions of the GPU cases of test_gpu_transd.py checked on the CPU."""
import numpy as np
import pytest
import torch

import transd_cases as tc
import transd_reference as tr
from helpers import golden, load

TIE_REL = 4e-6   # test_gpu_realscale.py's near-tie band, relative to max(1, |truth score|)


@pytest.mark.parametrize("path", golden("transd_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_gradients_match_reference_runs(path):
    """Every SGD lr 1 step of the reference: its table delta is the float64 gradient at the tables before it (to
    GRAD_DEV of the case's family, which this measures), its loss the float64 loss."""
    z = load(path)
    cfg = tr.golden_cfg(z)
    fam = tr.family(cfg)
    assert int(z["steps"]) >= 2 and float(z["lr"]) == 1.0
    for s in range(int(z["steps"])):
        before, after = tr.golden_tables(z, "s%d" % s), tr.golden_tables(z, "s%d" % (s + 1))
        (h, t, r), mode = tr.golden_step(z, cfg, s)
        loss, grads, aux = tr.loss_and_grads(before, h, t, r, cfg["batch_size"], cfg, mode)
        np.testing.assert_allclose(loss, float(z["losses"][s]), rtol=1e-6)
        dev = max(float(np.abs((before[i].astype(np.float64) - after[i].astype(np.float64)) - grads[i]).max())
                  for i in range(4))
        print("%s step %d: family %s GRAD_DEV %.3e (|g|max %.3e, active %.2f)"
              % (path.split("/")[-1], s, fam, dev, aux["gmax"], aux["active"]))
        assert dev <= tr.GRAD_DEV[fam], (fam, dev)


def test_grad_dev_table_covers_every_family():
    """Every family of the table is measured by a golden case: p 1 and 2, norm_flag on and off, normal and cross
    sampling, both init branches, dims from {8, 12, 16, 20}."""
    seen, combos, inits, dims = set(), set(), set(), set()
    for path in golden("transd_g*.npz"):
        cfg = tr.golden_cfg(load(path))
        seen.add(tr.family(cfg))
        combos.add((cfg["p_norm"], cfg["norm_flag"], cfg["sampling"]))
        inits.add(cfg["epsilon"] is not None)
        dims.add(cfg["dim"])
    assert seen == set(tr.GRAD_DEV)
    assert {c[0] for c in combos} == {1, 2} and {c[1] for c in combos} == {True, False}
    assert {c[2] for c in combos} == {"normal", "cross"}
    assert len(combos) == 8 and inits == {True, False} and dims == {8, 12, 16, 20}


@pytest.mark.parametrize("path", golden("transd_p*.npz"), ids=lambda p: p.split("/")[-1])
def test_predict_matches_reference(path):
    """The reference's predict in the three modes: the float64 distances to float32 rounding, and the float32
    evaluation of the same forward (what SCORE_DEV measures) to two ulps."""
    z = load(path)
    cfg = {"p_norm": int(z["p_norm"]), "norm_flag": bool(z["norm_flag"]), "dim": int(z["dim"])}
    tabs = tr.golden_tables(z, "")
    for mode in ("normal", "head_batch", "tail_batch"):
        h, t, r = tr.expand_predict(z[mode + "_h"], z[mode + "_t"], z[mode + "_r"], mode)
        want = z[mode + "_score"].astype(np.float64)
        ref = tr.scores(tabs, h, t, r, cfg, mode)
        got32 = tr.scores(tabs, h, t, r, cfg, mode, torch.float32).astype(np.float64)
        scale = np.maximum(1.0, ref)
        assert (np.abs(want - ref) / scale).max() <= 1e-6
        assert (np.abs(want - got32) / scale).max() <= 2 * 2.0 ** -23


def test_score_dev_is_measured():
    """SCORE_DEV again, from the float32 torch forward on the GPU score tests' inputs: not grown."""
    for D in tr.SCORE_DIMS:
        dev = tr.measure_score_dev(D)
        print("SCORE_DEV[%d] measured %.3e (table %.3e, tol %.3e)" % (D, dev, tr.SCORE_DEV[D], tr.score_tol(D)))
        assert dev <= tr.SCORE_DEV[D]


@pytest.mark.parametrize("path", golden("transd_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_optimizer_runs_match_reference(path):
    """The reference's Adam and Adagrad trajectories: float64 gradients + adam_update / the Adagrad formula from the
    recorded initial tables give its losses, its optimizer state after step 1 and at the end, and its final tables
    (Adam: to its per-step bound for two trajectories, 2 * steps * lr * (1 - beta1) / sqrt(1 - beta2); the final
    moments as test_adam_matches_reference_runs bounds them. Adagrad: state_sum = sum of g^2 to 2 |g|max GRAD_DEV per
    step plus an ulp, the tables to steps * lr * 1e-3)."""
    z = load(path)
    cfg = tr.golden_cfg(z)
    lr, steps, opt = float(z["lr"]), int(z["steps"]), str(z["optimizer"])
    w = [x.astype(np.float64) for x in tr.golden_tables(z, "init")]
    m = [np.zeros_like(x) for x in w]
    v = [np.zeros_like(x) for x in w]
    gmax = [0.0] * 4
    dev = max(tr.GRAD_DEV.values())
    for s in range(steps):
        (h, t, r), mode = tr.golden_step(z, cfg, s)
        loss, grads, _ = tr.loss_and_grads(w, h, t, r, cfg["batch_size"], cfg, mode)
        np.testing.assert_allclose(loss, float(z["losses"][s]), rtol=1e-4)
        for i in range(4):
            gmax[i] = max(gmax[i], float(np.abs(grads[i]).max()))
            if opt == "adam":
                w[i], m[i], v[i] = tr.adam_update(w[i], m[i], v[i], grads[i], lr, s + 1)
            else:
                v[i] = v[i] + grads[i] * grads[i]
                w[i] = w[i] - lr * grads[i] / (np.sqrt(v[i]) + 1e-10)
        if s == 0:
            for i, nm in enumerate(tr.TABLES):
                if opt == "adam":
                    np.testing.assert_allclose(m[i], z["step1_m_" + nm], rtol=0, atol=1e-7)
                    np.testing.assert_allclose(v[i], z["step1_v_" + nm], rtol=1e-4, atol=1e-12)
                else:
                    np.testing.assert_allclose(v[i], z["step1_sum_" + nm], rtol=1e-4, atol=1e-12)
    for i, nm in enumerate(tr.TABLES):
        if opt == "adam":
            cap = 2 * steps * lr * (1 - 0.9) / np.sqrt(1 - 0.999)
            dm = float(np.abs(m[i] - z["final_m_" + nm]).max())
            dv = float(np.abs(v[i] - z["final_v_" + nm]).max())
            v_bound = (1 - 0.999 ** steps) * 2 * gmax[i] * dev + 2.0 ** -23 * float(z["final_v_" + nm].max())
            print("%s %s: final |m - ref| %.3e (bound %.3e), |v - ref| %.3e (bound %.3e)"
                  % (path.split("/")[-1], nm, dm, dev, dv, v_bound))
            assert dm <= dev and dv <= v_bound
        else:
            cap = steps * lr * 1e-3
            dv = float(np.abs(v[i] - z["final_sum_" + nm]).max())
            v_bound = steps * (2 * gmax[i] * dev + 2.0 ** -23 * float(z["final_sum_" + nm].max()))
            print("%s %s: final |sum - ref| %.3e (bound %.3e)" % (path.split("/")[-1], nm, dv, v_bound))
            assert dv <= v_bound
        assert np.abs(w[i] - z["final_" + nm]).max() <= cap


def _fixture_models():
    """(fixture, constructor arguments) of every fixture that records freshly initialised tables."""
    out = []
    for path in golden("transd_g*.npz") + golden("transd_a*.npz"):
        z = load(path)
        cfg = tr.golden_cfg(z)
        out.append((path, z, "s0" if "s0_ent_embeddings" in z.files else "init", cfg["dim"], cfg["p_norm"],
                    cfg["norm_flag"], cfg["model_margin"], cfg["epsilon"], cfg["torch_seed"]))
    return out


def test_python_transd_matches_reference_construction():
    """torch.manual_seed(s); TransD(...) gives the reference's tables bit for bit in both init branches, and its
    state_dict keys; dim_e != dim_r raises."""
    from openke.module.model import TransD
    branches = set()
    for path, z, tag, dim, p, nf, gamma, eps, tseed in _fixture_models():
        want = tr.golden_tables(z, tag)
        torch.manual_seed(tseed)
        kge = TransD(ent_tot=want[0].shape[0], rel_tot=want[1].shape[0], dim_e=dim, dim_r=dim, p_norm=p,
                     norm_flag=nf, margin=gamma, epsilon=eps)
        branches.add(eps is not None)
        for name, w in zip(tr.TABLES, want):
            np.testing.assert_array_equal(getattr(kge, name).weight.detach().numpy(), w, err_msg=path)
        assert sorted(kge.state_dict().keys()) == [str(k) for k in z["state_keys"]]
        assert kge.margin_flag == (gamma is not None)
        assert [t is None for t in kge.tables()] == [False, False, True, False, False]
    assert branches == {True, False}
    seeded = TransD.seeded(int(load(golden("transd_g1.npz")[0])["torch_seed"]), 5, 2, dim_e=8, dim_r=8)
    torch.manual_seed(int(load(golden("transd_g1.npz")[0])["torch_seed"]))
    plain = TransD(5, 2, dim_e=8, dim_r=8)
    for a, b in zip(seeded.tables(), plain.tables()):
        assert a is None or torch.equal(a, b)
    with pytest.raises(NotImplementedError, match="dim_e != dim_r"):
        TransD(5, 2, dim_e=8, dim_r=12)


def test_parallel_universe_config_names_putransd():
    """Parallel_Universe_Config(embedding_model=TransD) fails with the PuTransD message, not an import error."""
    from openke.config import Parallel_Universe_Config
    from openke.module.model import TransD
    pu = object.__new__(Parallel_Universe_Config)
    pu.embedding_model = TransD
    with pytest.raises(NotImplementedError, match="PuTransD is not built yet"):
        pu._check_setup()


def test_lp_fixture_near_ties_are_rare():
    """transd_lp.npz: at most 2 % of the queries hold a candidate within TIE_REL of the truth's float64 score (the
    queries test_gpu_transd.py may excuse from rank equality)."""
    z = load(golden("transd_lp.npz")[0])
    cfg = {"p_norm": int(z["p_norm"]), "norm_flag": bool(z["norm_flag"]), "dim": int(z["dim"])}
    tabs = tr.golden_tables(z, "")
    q = z["queries"].astype(np.int64)
    excused = lp_excused(tabs, q, cfg)
    print("transd_lp: %d of %d (query, side) pairs hold a near tie" % (int(excused.sum()), excused.size))
    assert excused.any(axis=0).mean() <= 0.02


def lp_excused(tabs, q, cfg):
    """[2][n] whether query n's side holds a candidate other than the truth within TIE_REL of the truth's score."""
    out = np.zeros((2, len(q)), dtype=bool)
    for i, (h, t, r) in enumerate(q):
        for side, truth, anchor in ((0, h, t), (1, t, h)):
            s = tr.lp_scores(tabs, int(anchor), int(r), side, cfg)
            near = np.abs(s - s[truth]) <= TIE_REL * max(1.0, abs(s[truth]))
            out[side, i] = near.sum() > 1
    return out


@pytest.mark.parametrize("case", tc.ALL_CASES, ids=lambda c: c[0])
def test_gpu_case_input_conditions(case):
    """The seeds, margins and planted slots of the GPU cases, in float64: no component of v within 1e-6 of zero under
    p = 1, no hinge argument within 1e-5 of -m, no ||u|| under 1e-3, between 20 % and 80 % of the pairs active, every
    planted slot present."""
    tabs, (h, t, r), cfg, mode = tc.build(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    assert h.size == t.size == r.size == bs * (K + 1)
    assert h.min() >= 0 and t.min() >= 0 and max(h.max(), t.max()) < tr.E and 0 <= r.min() and r.max() < tr.R
    b = tc.as_batch((h, t, r), bs, mode)
    for x, y in zip(tr.expand_batch(b["batch_h"], b["batch_t"], b["batch_r"], mode, bs), (h, t, r)):
        np.testing.assert_array_equal(x, y)   # the mode's compact form holds the same slots
    loss, grads, aux = tr.loss_and_grads(tabs, h, t, r, bs, cfg, mode)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads)
    print("%s: active %.2f min|v| %.2e hinge gap %.2e min||u|| %.2e |g|max %.2e"
          % (case[0], aux["active"], aux["min_abs_v"], aux["hinge_gap"], aux["min_u"], aux["gmax"]))
    if cfg["p_norm"] == 1:
        assert aux["min_abs_v"] >= 1e-6, aux["min_abs_v"]
    assert aux["hinge_gap"] >= 1e-5, aux["hinge_gap"]
    assert aux["min_u"] >= 1e-3, aux["min_u"]
    assert 0.2 <= aux["active"] <= 0.8, aux["active"]
    flags = tc.planted(h, t, r, bs, K, mode)
    for k, v in flags.items():
        if k == "other_relation" and mode != "normal":
            assert not v   # head_batch / tail_batch broadcast the positive's relation
            continue
        assert v, k
    assert not grads[0][tc.FREE_ENT].any() and not grads[2][tc.FREE_ENT].any()
    assert not grads[1][tc.FREE_REL].any() and not grads[3][tc.FREE_REL].any()


@pytest.mark.parametrize("case", tc.ADAM_CASES, ids=lambda c: c[0])
def test_gpu_adam_case_inputs(case):
    """The Adam cases' batches: entity 35 is touched in step 1 only, entity 36 never; their rows start with zero
    moments; every step meets the input conditions of the gradient cases."""
    tabs, batches, cfg, (m0, v0), lr, step0 = tc.build_adam(case)
    bs = cfg["batch_size"]
    for s, (h, t, r) in enumerate(batches):
        ents = np.concatenate([h, t])
        assert (tc.ONCE_ENT in ents) == (s == 0) and tc.FREE_ENT not in ents
    for i in (0, 2):
        assert not m0[i][tc.ONCE_ENT:].any() and not v0[i][tc.ONCE_ENT:].any()
        assert m0[i][:tc.ONCE_ENT].any() and (v0[i][:tc.ONCE_ENT] > 0).all()
    h, t, r = batches[0]
    _, grads, aux = tr.loss_and_grads(tabs, h, t, r, bs, cfg)
    assert grads[0][tc.ONCE_ENT].any() and grads[2][tc.ONCE_ENT].any() and not grads[0][tc.FREE_ENT].any()
    if cfg["p_norm"] == 1:
        assert aux["min_abs_v"] >= 1e-6
    assert aux["hinge_gap"] >= 1e-5 and aux["min_u"] >= 1e-3 and 0.2 <= aux["active"] <= 0.8
