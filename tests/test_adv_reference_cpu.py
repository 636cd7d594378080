"""adv_reference.py (the float64 form of the weighted step and of dense Adam) against the reference implementation's
own float32 runs (tests/golden/adv_*.npz, written by tests/golden/make_golden_adv.py), and the input conditions of
the GPU cases of test_gpu_adv.py checked on the CPU."""
import numpy as np
import pytest

import adv_cases
import adv_reference as ar
from helpers import golden, load


def _step(z, cfg, s):
    bs = cfg["batch_size"]
    return ar.expand_batch(z["b%d_h" % s], z["b%d_t" % s], z["b%d_r" % s], str(z["modes"][s]), bs)


@pytest.mark.parametrize("path", golden("adv_g*.npz"), ids=lambda p: p.split("/")[-1])
def test_gradients_match_reference_runs(path):
    """Every SGD lr 1 step of the reference: its table delta is the float64 gradient at the tables before it (to
    GRAD_DEV of the case's family, which this measures), its loss the float64 loss."""
    z = load(path)
    cfg = ar.golden_cfg(z)
    fam = ar.family(cfg)
    assert int(z["steps"]) >= 1 and float(z["lr"]) == 1.0
    for s in range(int(z["steps"])):
        before, after = ar.golden_tables(z, "s%d" % s), ar.golden_tables(z, "s%d" % (s + 1))
        h, t, r = _step(z, cfg, s)
        loss, grads, aux = ar.loss_and_grads(before, h, t, r, cfg["batch_size"], cfg)
        np.testing.assert_allclose(loss, float(z["losses"][s]), rtol=1e-6)
        dev = max(float(np.abs((before[i].astype(np.float64) - after[i].astype(np.float64)) - grads[i]).max())
                  for i in range(2))
        print("%s step %d: family %s GRAD_DEV %.3e (|g|max %.3e)" % (path.split("/")[-1], s, fam, dev, aux["gmax"]))
        assert dev <= ar.GRAD_DEV[fam], (fam, dev)


def test_grad_dev_table_covers_every_family():
    """Every family of the table is measured by a golden case: the sigmoid and margin losses with and without the
    adversarial weights, p 1 and 2, norm_flag on and off, normal and cross sampling."""
    seen = set()
    combos = set()
    for path in golden("adv_g*.npz"):
        cfg = ar.golden_cfg(load(path))
        seen.add(ar.family(cfg))
        combos.add((cfg["p_norm"], cfg["norm_flag"], cfg["sampling"]))
    assert seen == set(ar.GRAD_DEV)
    assert {c[0] for c in combos} == {1, 2} and {c[1] for c in combos} == {True, False}
    assert {c[2] for c in combos} == {"normal", "cross"}


@pytest.mark.parametrize("path", golden("adv_a*.npz"), ids=lambda p: p.split("/")[-1])
def test_adam_matches_reference_runs(path):
    """The reference's Adam trajectories: float64 gradients + adam_update from the recorded initial tables give
    its losses, its exp_avg / exp_avg_sq after step 1 and at the end, and its final tables (to Adam's per-step
    bound for two trajectories, 2 * steps * lr * (1 - beta1) / sqrt(1 - beta2)). The final moments pin the 10-step
    recursion: exp_avg is a weighted mean of the gradients, so it is off by at most the gradients' own deviation
    (the largest GRAD_DEV); exp_avg_sq = (1 - b2) sum b2^k g^2 by at most (1 - b2^steps) 2 |g|max GRAD_DEV plus one
    float32 ulp of its largest value."""
    z = load(path)
    cfg = ar.golden_cfg(z)
    lr, steps = float(z["lr"]), int(z["steps"])
    names = ["ent_embeddings", "rel_embeddings"] + (["norm_vector"] if cfg["model"] == "TransH" else [])
    w = [x.astype(np.float64) for x in ar.golden_tables(z, "init") if x is not None]
    m = [np.zeros_like(x) for x in w]
    v = [np.zeros_like(x) for x in w]
    gmax = [0.0] * len(w)
    for s in range(steps):
        h, t, r = _step(z, cfg, s)
        loss, grads, _ = ar.loss_and_grads(w, h, t, r, cfg["batch_size"], cfg)
        np.testing.assert_allclose(loss, float(z["losses"][s]), rtol=1e-4)
        for i in range(len(w)):
            gmax[i] = max(gmax[i], float(np.abs(grads[i]).max()))
            w[i], m[i], v[i] = ar.adam_update(w[i], m[i], v[i], grads[i], lr, s + 1)
        if s == 0:
            for i, nm in enumerate(names):
                np.testing.assert_allclose(m[i], z["step1_m_" + nm], rtol=0, atol=1e-7)
                np.testing.assert_allclose(v[i], z["step1_v_" + nm], rtol=1e-4, atol=1e-12)
    cap = 2 * steps * lr * (1 - 0.9) / np.sqrt(1 - 0.999)
    for i, nm in enumerate(names):
        assert np.abs(w[i] - z["final_" + nm]).max() <= cap
        dev = max(ar.GRAD_DEV.values())
        dm = float(np.abs(m[i] - z["final_m_" + nm]).max())
        dv = float(np.abs(v[i] - z["final_v_" + nm]).max())
        v_bound = (1 - 0.999 ** steps) * 2 * gmax[i] * dev + 2.0 ** -23 * float(z["final_v_" + nm].max())
        print("%s %s: final |m - ref| %.3e (bound %.3e), |v - ref| %.3e (bound %.3e)"
              % (path.split("/")[-1], nm, dm, dev, dv, v_bound))
        assert dm <= dev
        assert dv <= v_bound


@pytest.mark.parametrize("case", adv_cases.ALL_CASES, ids=lambda c: c[0])
def test_gpu_case_input_conditions(case):
    """The seeds of the GPU cases: in float64 no slot has a component of v within 1e-6 of zero under p = 1 (a sign
    flip there is no path bug), no hinge argument lies within 1e-5 of -m, and the batch is valid."""
    tabs, batch, cfg = adv_cases.build(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    h, t, r = ar.expand_batch(batch["batch_h"], batch["batch_t"], batch["batch_r"], batch["mode"], bs)
    assert h.size == t.size == r.size == bs * (K + 1)
    assert h.min() >= 0 and t.min() >= 0 and max(h.max(), t.max()) < adv_cases.E and 0 <= r.min() and r.max() < adv_cases.R
    loss, grads, aux = ar.loss_and_grads(tabs, h, t, r, bs, cfg)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads)
    if cfg["p_norm"] == 1:
        assert aux["min_abs_v"] >= 1e-6, aux["min_abs_v"]
    assert aux["hinge_gap"] >= 1e-5, aux["hinge_gap"]
    if bs * K >= 6:
        # repeated corrupted entities are certain with six entities; a negative equal to one of the positive's rows too
        hn, tn = h[bs:].reshape(K, bs), t[bs:].reshape(K, bs)
        assert ((hn == h[:bs]) | (tn == t[:bs])).any()


def test_stability_case_shape():
    """The stability case: distances around 30 at temperature 40 with unnormalised rows scaled by 8."""
    tabs, batch, cfg = adv_cases.build(adv_cases.STABILITY_CASE)
    bs = cfg["batch_size"]
    h, t, r = ar.expand_batch(batch["batch_h"], batch["batch_t"], batch["batch_r"], batch["mode"], bs)
    _, _, aux = ar.loss_and_grads(tabs, h, t, r, bs, cfg)
    assert cfg["adv_temperature"] == 40.0 and not cfg["norm_flag"]
    assert 20.0 <= float(np.median(aux["d"])) <= 40.0 and aux["d"].max() >= 30.0


@pytest.mark.parametrize("case", adv_cases.ADAM_CASES, ids=lambda c: c[0])
def test_gpu_adam_case_inputs(case):
    """The Adam cases' batches: entity 6 is touched in step 1 only, entity 7 never; rows 6 and 7 start with zero
    moments; the first step meets the input conditions of the gradient cases."""
    tabs, batches, cfg, (m0, v0), lr, step0 = adv_cases.build_adam(case)
    bs = cfg["batch_size"]
    for s, b in enumerate(batches):
        ents = np.concatenate([b["batch_h"], b["batch_t"]])
        assert (6 in ents) == (s == 0) and 7 not in ents
    assert not m0[0][6:].any() and not v0[0][6:].any() and m0[0][:6].any() and (v0[0][:6] > 0).all()
    b = batches[0]
    _, grads, aux = ar.loss_and_grads([x for x in tabs if x is not None],
                                      *ar.expand_batch(b["batch_h"], b["batch_t"], b["batch_r"], "normal", bs), bs, cfg)
    assert grads[0][6].any() and not grads[0][7].any()
    if cfg["p_norm"] == 1:
        assert aux["min_abs_v"] >= 1e-6
    assert aux["hinge_gap"] >= 1e-5
