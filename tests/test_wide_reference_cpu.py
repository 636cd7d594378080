"""CPU side of the wide-dim tests (TransE / TransH single models at dims 516..1024): the dim rule of the library, the
two deviation tables of wide_cases.py measured again, the float32 form behind GRAD_DEV_WIDE pinned to one recorded
step of the reference implementation at dim 1024 (tests/golden/wide_g1.npz, written by
tests/golden/make_golden_wide.py), and the input conditions of the GPU cases of test_gpu_wide.py."""
import numpy as np
import pytest

import adv_reference as ar
import oracle
import wide_cases as wc
from conftest import KG_SMALL
from helpers import golden, load
from lp_reference import TOL_CAP
from test_lp_reference_cpu import _deviation


def test_model_dim_rule():
    """pt_model_dim_supported over 1..1100: TransE / TransH at dims 1..512 and at multiples of 4 from 516 to 1024,
    TransD at 1..512, nothing else; no model but the three."""
    from openke import _native
    L = _native.lib()
    for model in (_native.PT_TRANSE, _native.PT_TRANSH, _native.PT_TRANSD):
        wide = model != _native.PT_TRANSD
        for dim in range(-1, 1101):
            want = 1 <= dim <= 512 or (wide and 516 <= dim <= 1024 and dim % 4 == 0)
            assert L.pt_model_dim_supported(dim, model) == int(want), (dim, model)
    assert L.pt_model_dim_supported(2048, _native.PT_TRANSE) == 0
    assert L.pt_model_dim_supported(8, 3) == 0 and L.pt_model_dim_supported(8, -1) == 0
    # the universe trainer's own rule is untouched: float4 rows up to 1,024, no TransD
    assert L.pt_universe_dim_supported(1024, _native.PT_TRANSE) == 1
    assert L.pt_universe_dim_supported(20, _native.PT_TRANSD) == 0


@pytest.mark.parametrize("D", wc.WIDE_DIMS)
def test_oracle_deviation_within_table(D):
    """ORACLE_DEV_WIDE measured as lp_reference.ORACLE_DEV is; four times it stays under the 1e-5 cap."""
    dev, where = _deviation(D)
    print("ORACLE_DEV_WIDE D %d: measured %.3e at %s, table %.3e, tol %.3e" % (D, dev, where, wc.ORACLE_DEV_WIDE[D],
                                                                                wc.score_tol(D)))
    assert dev <= wc.ORACLE_DEV_WIDE[D], (D, dev, where)
    assert wc.ORACLE_DEV_WIDE[D] <= (D + 16) * 2.0 ** -24, (D, wc.ORACLE_DEV_WIDE[D])
    assert 4 * wc.ORACLE_DEV_WIDE[D] < TOL_CAP


def test_grad_deviation_within_table():
    """GRAD_DEV_WIDE measured again on the GPU tests' own inputs, per family; four times it stays under the cap."""
    worst = {}
    for fam, name, tabs, hrt, bs, cfg in wc.gradient_inputs():
        dev = wc.grad_dev(tabs, *hrt, bs, cfg)
        if dev > worst.get(fam, (0.0, None))[0]:
            worst[fam] = (dev, name)
    assert set(worst) == set(wc.GRAD_DEV_WIDE)
    for fam, (dev, name) in sorted(worst.items()):
        print("GRAD_DEV_WIDE %s: measured %.3e at %s, table %.3e" % (fam, dev, name, wc.GRAD_DEV_WIDE[fam]))
        assert dev <= wc.GRAD_DEV_WIDE[fam], (fam, dev, name)
        assert 4 * wc.GRAD_DEV_WIDE[fam] < TOL_CAP


def test_float32_form_matches_the_reference_run():
    """wide_g1.npz: the reference's TransE at dim 1024 under SigmoidLoss(adv_temperature=1), one SGD lr 1 step on
    kg_small, touched rows only. Its table delta is the float32 torch evaluation of adv_reference's forward to the
    rounding of w - g, its loss the float64 loss; what it deviates from float64 is printed beside the float32 form's
    deviation."""
    z = load(golden("wide_g1.npz")[0])
    cfg = ar.golden_cfg(z)
    assert cfg["dim"] == 1024 and cfg["loss"] == "sigmoid" and cfg["adv_temperature"] == 1.0 and float(z["lr"]) == 1.0
    names = ("ent_embeddings", "rel_embeddings")
    maps = [{int(g): i for i, g in enumerate(z["rows_" + k])} for k in names]
    h, t = (np.array([maps[0][int(x)] for x in z[k]]) for k in ("b_h", "b_t"))
    r = np.array([maps[1][int(x)] for x in z["b_r"]])
    tabs = [z["s0_" + k] for k in names]
    bs = cfg["batch_size"]
    loss, g64, aux = ar.loss_and_grads(tabs, h, t, r, bs, cfg)
    g32 = wc.grads32(tabs, h, t, r, bs, cfg)
    np.testing.assert_allclose(loss, float(z["losses"][0]), rtol=1e-6)
    for i, k in enumerate(names):
        delta = z["s0_" + k].astype(np.float64) - z["s1_" + k].astype(np.float64)
        rounding = float(np.spacing(np.float32(np.abs(tabs[i]).max() + np.abs(g64[i]).max())))
        d_ref32, d_ref64, d_3264 = (float(np.abs(a - b).max()) for a, b in ((delta, g32[i]), (delta, g64[i]),
                                                                             (g32[i], g64[i])))
        print("%s: |ref - f32| %.3e (rounding of w - g %.3e), |ref - f64| %.3e, |f32 - f64| %.3e, |g|max %.3e"
              % (k, d_ref32, rounding, d_ref64, d_3264, float(np.abs(g64[i]).max())))
        assert d_ref32 <= rounding
        assert d_ref64 <= wc.GRAD_DEV_WIDE[ar.family(cfg)]


def _check_conditions(name, tabs, hrt, bs, cfg):
    loss, grads, aux = wc.conditions(tabs, *hrt, bs, cfg)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads)
    print("%s: active %.2f min|v| %.2e hinge gap %.2e |g|max %.2e" % (name, aux["active"], aux["min_abs_v"],
                                                                     aux["hinge_gap"], aux["gmax"]))
    if cfg["p_norm"] == 1:
        assert aux["min_abs_v"] >= 1e-6, aux["min_abs_v"]
    if cfg["loss"] == "margin":
        assert aux["hinge_gap"] >= 1e-5, aux["hinge_gap"]
        assert 0.2 <= aux["active"] <= 0.8, aux["active"]
    return grads


@pytest.mark.parametrize("case", wc.PLAIN_CASES, ids=lambda c: c[0])
def test_plain_case_input_conditions(case):
    """Between 20 % and 80 % of the pairs active, no |v| component under 1e-6 at p = 1, no hinge argument within 1e-5
    of its kink, every planted slot present, the free rows without a gradient."""
    tabs, hrt, cfg = wc.build_plain(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    assert all(len(x) == bs * (K + 1) for x in hrt)
    flags = wc.planted(*hrt, bs, K)
    assert all(flags.values()), flags
    grads = _check_conditions(case[0], tabs, hrt, bs, cfg)
    assert not grads[0][wc.FREE_ENT].any() and not any(g[wc.FREE_REL].any() for g in grads[1:])


@pytest.mark.parametrize("case", wc.ADV_CASES + wc.STABILITY_CASES, ids=lambda c: c[0])
def test_weighted_case_input_conditions(case):
    tabs, batch, cfg = wc.build_adv(case)
    bs = cfg["batch_size"]
    _check_conditions(case[0], tabs, wc.expanded(batch, bs), bs, cfg)
    assert ar.family(cfg) in wc.GRAD_DEV_WIDE


def test_weighted_cases_cover_the_families_of_the_small_dims():
    import adv_cases
    small = {ar.family(adv_cases.case_cfg(c)) for c in adv_cases.GRAD_CASES}
    for D in wc.WIDE_DIMS:
        assert {ar.family(adv_cases.case_cfg(c)) for c in wc.ADV_CASES if c[1] == D} == small
    assert {c[3] for c in wc.ADV_CASES} == {3, 7, 70} and all(c[8] == 40.0 for c in wc.STABILITY_CASES)


@pytest.mark.parametrize("case", wc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_case_inputs(case):
    """Entity 68 is touched in step 1 only, entity 69 never; their rows start with zero moments; every step meets the
    input conditions of the gradient cases."""
    tabs, batches, cfg, (m0, v0), lr, step0 = wc.build_adam(case)
    bs = cfg["batch_size"]
    for s, b in enumerate(batches):
        hrt = wc.expanded(b, bs)
        ents = np.concatenate(hrt[:2])
        assert (wc.ONCE_ENT in ents) == (s == 0) and wc.FREE_ENT not in ents
        grads = _check_conditions("%s step %d" % (case[0], s), tabs, hrt, bs, cfg)
        assert grads[0][wc.ONCE_ENT].any() == (s == 0) and not grads[0][wc.FREE_ENT].any()
    assert not m0[0][wc.ONCE_ENT:].any() and not v0[0][wc.ONCE_ENT:].any()
    assert m0[0][:wc.ONCE_ENT].any() and (v0[0][:wc.ONCE_ENT] > 0).all()


def _lp_fixture(case):
    kg = oracle.KG.load(KG_SMALL)
    tabs = wc.lp_tables(case, kg.ent_total, kg.rel_total)
    h, t, r = oracle.sort_test(*oracle.read_triples(KG_SMALL + "test2id.txt"))
    return kg, tabs, (h, t, r), wc.lp_rows64(case, tabs, h, t, r)


@pytest.mark.parametrize("case", wc.LP_CASES, ids=lambda c: "%s-d%d" % c[:2])
def test_lp_fixture_near_ties_are_rare(case):
    """At most 2 % of the queries hold a candidate within tol(D) of the truth's float64 score (the queries
    test_gpu_wide.py may excuse from rank equality), and wide_cases.ranks_from_rows is the oracle's ranking: equal to
    oracle.link_prediction on the same rows rounded to float32."""
    kg, tabs, (h, t, r), (rows_h, rows_t) = _lp_fixture(case)
    near = wc.lp_near_ties(case, rows_h, rows_t, h, t)
    print("%s d%d: %d of %d (query, side) pairs hold a near tie" % (case[0], case[1], int(near.sum()), near.size))
    assert near.any(axis=0).mean() <= 0.02
    all_tr = [np.concatenate(x) for x in zip(*(oracle.read_triples(KG_SMALL + f)
                                              for f in ("test2id.txt", "train2id.txt", "valid2id.txt")))]
    known = set(zip(*(x.tolist() for x in all_tr)))
    E = kg.ent_total
    r32_h, r32_t = rows_h.astype(np.float32), rows_t.astype(np.float32)
    con_h = np.stack([r32_h[i][oracle.candidates(E, int(h[i]))] for i in range(len(h))])
    con_t = np.stack([r32_t[i][oracle.candidates(E, int(t[i]))] for i in range(len(h))])
    _, want = oracle.link_prediction(E, all_tr, (h, t, r), con_h, con_t)
    got = wc.ranks_from_rows(r32_h.astype(np.float64), r32_t.astype(np.float64), h, t, r, known)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
