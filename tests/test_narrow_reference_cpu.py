"""CPU side of tests/test_gpu_narrow.py: the input conditions of every case of narrow_cases.py, which k_step_sampled
instance each sampled case selects (with the coverage the case list claims), and the deviation tables of
narrow_cases.py measured again."""
import numpy as np
import pytest

import adv_reference as ar
import narrow_cases as nc
import transd_cases as tc
import transd_reference as tr
import wide_cases as wc
from lp_reference import TOL_CAP
from test_lp_reference_cpu import _deviation


# ------------------------------------------------------------------ kernel selection ------------
def test_selection_restates_the_launcher():
    """pick_shape at the dims the issue of these tests names, pick_nch, and PT_SSHAPES as parsed."""
    assert [nc.pick_shape(D) for D in (1, 2, 3, 9, 15, 129, 255, 257, 511)] == [
        (2, 1, 1), (2, 1, 1), (4, 1, 1), (16, 1, 1), (16, 1, 1), (64, 1, 4), (64, 1, 4), (64, 1, 8), (64, 1, 8)]
    assert nc.pick_shape(200) == (64, 4, 1) and nc.pick_shape(200, False) == (64, 1, 4)
    assert nc.pick_shape(300, False) == (64, 1, 8) and nc.pick_shape(512, False) == (64, 1, 8)
    assert nc.pick_shape(1024) == (64, 4, 4) and nc.pick_shape(516) == (64, 4, 3)
    assert [nc.pick_nch(n, 1) for n in (1, 2, 4, 5, 8, 9, 35)] == [1, 4, 4, 8, 8, 32, 32]
    assert [nc.pick_nch(n, 8) for n in (1, 3, 6, 10)] == [1, 4, 8, 8] and nc.pick_nch(10, 4) == 32
    listed = nc.sshapes()
    assert len(listed) == 45 and len(set(listed)) == 45 and all(s[1] == 1 for s in listed)
    assert (64, 1, 4, 4, 4) in listed and (64, 1, 8, 32, 4) not in listed and (64, 1, 8, 4, 4) not in listed
    # (64,1,8) at neg 8: two per sub-group prefer NCH 4, which has no S = 4 instance there: the fallback takes NCH 8
    assert nc.sampled_instance("TransH", 511, 8, listed) == (64, 1, 8, 8, 4, True)
    assert not nc.reaches_sampled("TransE", 300, 4) and nc.reaches_sampled("TransE", 300, 3)
    assert nc.reaches_sampled("TransH", 300, 4) and nc.reaches_sampled("TransE", 301, 4)


def test_sampled_cases_select_listed_instances_and_cover_them():
    """Every sampled case runs k_step_sampled, at an instance of PT_SSHAPES; for each model the cases cover every
    (G, KCH) pair a dim 1..512 selects and every (NCH, S) column, and the list holds what it was written for."""
    listed = nc.sshapes()
    names = [nc.sampled_name(c) for c in nc.SAMPLED_CASES]
    assert len(set(names)) == len(names)
    seen = {"TransE": set(), "TransH": set()}
    for case in nc.SAMPLED_CASES:
        model, D, p, nf, opt, bs, neg, bern, filt, steps = case
        assert nc.reaches_sampled(model, D, neg), case
        inst = nc.sampled_instance(model, D, neg, listed)
        print("%-40s k_step_sampled<%d, G %d, VEC %d, KCH %d, NCH %d, S %d, CSR %d>, %d step(s)"
              % ((nc.sampled_name(case), model == "TransH") + inst + (steps,)))
        assert inst is not None and inst[:5] in listed, case
        assert bs <= 48 and 1 <= steps <= 3
        seen[model].add(inst)
    pairs = {nc.pick_shape(D, False)[::2] for D in range(1, 513)}
    assert pairs == {(s[0], s[2]) for s in listed}
    columns = {(s[3], s[4]) for s in listed}
    assert columns == {(1, 1), (4, 1), (8, 1), (8, 4), (32, 4), (4, 4)}
    for model, insts in seen.items():
        assert {(i[0], i[2]) for i in insts} == pairs, (model, pairs - {(i[0], i[2]) for i in insts})
        assert {(i[3], i[4]) for i in insts} == columns, model
        assert {i[5] for i in insts} == {True, False}
    # what the list was written for
    has = {(c[0], c[1], c[6]) for c in nc.SAMPLED_CASES}
    for model in ("TransE", "TransH"):
        assert {D for m, D, _ in has if m == model} >= {3, 13, 130, 255, 257, 511}
    assert {("TransH", 200), ("TransH", 512)} <= {(m, D) for m, D, _ in has} and ("TransE", 300, 2) in has
    for kch in (4, 8):   # the negative counts at the two wide one-float shapes
        negs = {n for _, D, n in has if nc.pick_shape(D, False) == (64, 1, kch)}
        assert negs >= {1, 3, 6, 8, 9, 10}, (kch, negs)
    assert any(nc.pick_shape(D, False)[2] == 8 and n == 40 for _, D, n in has)
    assert ("TransE", 13, 140) in has
    assert ("TransE", 3, 24, 8) in {(c[0], c[1], c[5], c[6]) for c in nc.SAMPLED_CASES}
    wide_h = {(c[1], c[3]) for c in nc.SAMPLED_CASES if c[0] == "TransH" and c[6] >= 8}
    assert len({D for D, _ in wide_h}) >= 3 and {nf for _, nf in wide_h} == {True, False}
    assert {c[2] for c in nc.SAMPLED_CASES} == {1, 2} and {c[3] for c in nc.SAMPLED_CASES} == {True, False}
    assert sum(1 for c in nc.SAMPLED_CASES if not c[7]) >= 2 and sum(1 for c in nc.SAMPLED_CASES if not c[8]) >= 2
    assert sum(1 for c in nc.SAMPLED_CASES if c[7] and c[8]) > len(nc.SAMPLED_CASES) // 2
    ada = sum(1 for c in nc.SAMPLED_CASES if c[4] == "adagrad")
    assert 0.25 <= ada / len(nc.SAMPLED_CASES) <= 0.45, ada


# ------------------------------------------------------------------ input conditions ------------
def _check_conditions(name, aux, cfg, loss, grads):
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads)
    print("%s: active %.2f min|v| %.2e hinge gap %.2e |g|max %.2e" % (name, aux["active"], aux["min_abs_v"],
                                                                     aux["hinge_gap"], aux["gmax"]))
    if cfg["p_norm"] == 1:
        assert aux["min_abs_v"] >= 1e-6, aux["min_abs_v"]
    if cfg["loss"] == "margin":
        assert aux["hinge_gap"] >= 1e-5, aux["hinge_gap"]
        assert 0.2 <= aux["active"] <= 0.8, aux["active"]


@pytest.mark.parametrize("case", nc.SAMPLED_CASES, ids=nc.sampled_name)
def test_sampled_case_input_conditions(case):
    """Every step's batch: between 20 % and 80 % of the pairs active, no |v| component under 1e-6 at p = 1, no hinge
    argument within 1e-5 of its kink, TransH's projections well conditioned; the batch is the oracle's sampling() in
    the expanded layout, and a row no slot names has no gradient."""
    model, D, p, nf, opt, bs, neg, bern, filt, steps = case
    b = nc.build_sampled(case)
    assert len(b["steps"]) == steps and len(b["states"]) == steps + 1
    assert b["cfg"]["loss_margin"] == nc.margin(p, nf, D) and b["cfg"]["plain"]
    for k, s in enumerate(b["steps"]):
        h, t, r = s["hrt"]
        assert h.size == t.size == r.size == bs * (neg + 1)
        assert (np.tile(r[:bs], neg + 1) == r).all()   # entity corruptions only
        _check_conditions("%s step %d" % (b["name"], k), s["aux"], b["cfg"], s["loss"], s["grads"])
        assert nc.well_conditioned(model, nf, b["tabs"], np.concatenate([h, t]), r)
        free_e = np.setdiff1d(np.arange(b["tabs"][0].shape[0]), np.concatenate([h, t]))
        free_r = np.setdiff1d(np.arange(b["tabs"][1].shape[0]), r)
        assert free_e.size and not s["grads"][0][free_e].any()
        assert all(not g[free_r].any() for g in s["grads"][1:])
        assert (b["states"][k] != b["states"][k + 1]).any()


@pytest.mark.parametrize("case", nc.PLAIN_CASES, ids=lambda c: c[0])
def test_plain_case_input_conditions(case):
    tabs, hrt, cfg = nc.build_plain(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    assert all(len(x) == bs * (K + 1) for x in hrt)
    flags = wc.planted(*hrt, bs, K)
    assert all(flags.values()), flags
    loss, grads, aux = wc.conditions(tabs, *hrt, bs, cfg)
    _check_conditions(case[0], aux, cfg, loss, grads)
    assert nc.well_conditioned(case[1], case[5], tabs, np.concatenate(hrt[:2]), hrt[2])
    assert not (case[1] == "TransH" and case[2] == 2 and case[5])
    assert not grads[0][wc.FREE_ENT].any() and not any(g[wc.FREE_REL].any() for g in grads[1:])


def test_plain_cases_cover_dims_models_and_optimizers():
    assert {(c[2], c[1], c[7]) for c in nc.PLAIN_CASES} == {(D, m, o) for D in nc.NARROW_DIMS
                                                            for m in ("TransE", "TransH") for o in ("sgd", "adagrad")}
    assert {(c[3], c[4]) for c in nc.PLAIN_CASES} == {(11, 3), (37, 7)}
    for D in nc.NARROW_DIMS:
        assert {c[6] for c in nc.PLAIN_CASES if c[2] == D} == {1, 2}
        assert nc.pick_shape(D) in ((2, 1, 1), (4, 1, 1), (16, 1, 1), (64, 1, 4), (64, 1, 8))
    assert {nc.pick_shape(D) for D in nc.NARROW_DIMS} == {(2, 1, 1), (4, 1, 1), (16, 1, 1), (64, 1, 4), (64, 1, 8)}


@pytest.mark.parametrize("case", nc.ADV_CASES, ids=lambda c: c[0])
def test_weighted_case_input_conditions(case):
    tabs, batch, cfg = wc.build_adv(case)
    bs = cfg["batch_size"]
    loss, grads, aux = wc.conditions(tabs, *wc.expanded(batch, bs), bs, cfg)
    _check_conditions(case[0], aux, cfg, loss, grads)
    assert nc.family(cfg) in nc.GRAD_DEV_NARROW


def test_weighted_cases_cover_the_families_of_the_small_dims():
    import adv_cases
    small = {ar.family(adv_cases.case_cfg(c)) for c in adv_cases.GRAD_CASES}
    for D in (130, 257):
        for K in (3, 70):
            assert {ar.family(adv_cases.case_cfg(c)) for c in nc.ADV_CASES if c[1] == D and c[3] == K} == small


@pytest.mark.parametrize("case", nc.ADAM_CASES, ids=lambda c: c[0])
def test_adam_case_inputs(case):
    """Entity 68 is touched in step 1 only, entity 69 never; their rows start with zero moments; every step meets the
    input conditions of the gradient cases."""
    tabs, batches, cfg, (m0, v0), lr, step0 = wc.build_adam(case)
    bs = cfg["batch_size"]
    assert nc.well_conditioned(case[1], case[5], tabs)
    for s, b in enumerate(batches):
        hrt = wc.expanded(b, bs)
        ents = np.concatenate(hrt[:2])
        assert (wc.ONCE_ENT in ents) == (s == 0) and wc.FREE_ENT not in ents
        loss, grads, aux = wc.conditions(tabs, *hrt, bs, cfg)
        _check_conditions("%s step %d" % (case[0], s), aux, cfg, loss, grads)
        assert grads[0][wc.ONCE_ENT].any() == (s == 0) and not grads[0][wc.FREE_ENT].any()
    assert not m0[0][wc.ONCE_ENT:].any() and not v0[0][wc.ONCE_ENT:].any()
    assert m0[0][:wc.ONCE_ENT].any() and (v0[0][:wc.ONCE_ENT] > 0).all()


@pytest.mark.parametrize("case", nc.TRANSD_CASES, ids=lambda c: c[0])
def test_transd_case_input_conditions(case):
    """test_transd_reference_cpu.test_gpu_case_input_conditions at the three dims."""
    tabs, (h, t, r), cfg, mode = tc.build(case)
    bs, K = cfg["batch_size"], cfg["neg_ent"]
    assert h.size == t.size == r.size == bs * (K + 1)
    loss, grads, aux = tr.loss_and_grads(tabs, h, t, r, bs, cfg, mode)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads)
    print("%s: active %.2f min|v| %.2e hinge gap %.2e min||u|| %.2e |g|max %.2e"
          % (case[0], aux["active"], aux["min_abs_v"], aux["hinge_gap"], aux["min_u"], aux["gmax"]))
    if cfg["p_norm"] == 1:
        assert aux["min_abs_v"] >= 1e-6, aux["min_abs_v"]
    assert aux["hinge_gap"] >= 1e-5 and aux["min_u"] >= 1e-3 and 0.2 <= aux["active"] <= 0.8
    for k, v in tc.planted(h, t, r, bs, K, mode).items():
        assert v == (not (k == "other_relation" and mode != "normal")), k
    assert not grads[0][tc.FREE_ENT].any() and not grads[2][tc.FREE_ENT].any()
    assert not grads[1][tc.FREE_REL].any() and not grads[3][tc.FREE_REL].any()
    assert {c[1] for c in nc.TRANSD_CASES} == set(nc.TRANSD_DIMS) and nc.family(cfg) in nc.GRAD_DEV_NARROW


@pytest.mark.parametrize("model", ["TransE", "TransH"])
@pytest.mark.parametrize("D", nc.NARROW_DIMS)
def test_score_inputs_are_well_conditioned(D, model):
    """TransH under norm_flag: no entity of the score and link-prediction tables within MIN_PROJECTED of a relation's
    normal (every row is scored against every relation there)."""
    for p in (1, 2):
        for nf in (True, False):
            tabs, batches = nc.score_case(model, D, p, nf)
            assert set(batches) == {"normal", "head_batch", "tail_batch"}
            assert nc.well_conditioned(model, nf, tabs)
            u, pairs = nc.lp_case(model, D, p, nf)
            assert u["ent"].shape == (nc.LP_E_LOCAL, D) and len({k for k, _, _, _, _ in pairs}) == nc.LP_KEYS
            assert {s for _, _, _, _, s in pairs} == {0, 1}
            assert nc.well_conditioned(model, nf, [u["ent"], u["rel"], u["normv"]])
            if model == "TransH" and nf:
                print("%s D %d p %d: smallest |e_perp| / |e| %.3f (scores), %.3f (link prediction)"
                      % (model, D, p, nc.projected_share(tabs[0], tabs[2]), nc.projected_share(u["ent"], u["normv"])))


# ------------------------------------------------------------------ deviation tables ------------
@pytest.mark.parametrize("D", nc.NARROW_DIMS)
def test_oracle_deviation_within_table(D):
    """ORACLE_DEV measured as lp_reference.ORACLE_DEV is. From dim 13 on four times it stays under the 1e-5 cap and
    the entry within (D + 16) ulp; at dims 2 and 3 it is TransH with norm_flag on unconditioned inputs that decides
    (narrow_cases.MIN_PROJECTED), and the cap is the tolerance."""
    dev, where = _deviation(D)
    print("ORACLE_DEV D %d: measured %.3e at %s, table %.3e, tol %.3e" % (D, dev, where, nc.ORACLE_DEV[D],
                                                                          nc.score_tol(D)))
    assert dev <= nc.ORACLE_DEV[D], (D, dev, where)
    if D >= 13:
        assert nc.ORACLE_DEV[D] <= (D + 16) * 2.0 ** -24, (D, nc.ORACLE_DEV[D])
        assert 4 * nc.ORACLE_DEV[D] < TOL_CAP
    else:
        assert where == ("TransH", where[1], 1) and nc.score_tol(D) == TOL_CAP


def test_transd_score_deviation_within_table():
    for D in nc.TRANSD_DIMS:
        dev = tr.measure_score_dev(D)
        print("SCORE_DEV[%d] measured %.3e (table %.3e, tol %.3e)" % (D, dev, nc.SCORE_DEV[D], nc.transd_score_tol(D)))
        assert dev <= nc.SCORE_DEV[D] and 4 * nc.SCORE_DEV[D] < TOL_CAP


def test_grad_deviation_within_table():
    """GRAD_DEV_NARROW measured again on the GPU tests' own inputs, per family; four times it stays under the cap."""
    worst = {}
    for fam, name, measure in nc.gradient_inputs():
        dev = measure()
        if dev > worst.get(fam, (-1.0, None))[0]:
            worst[fam] = (dev, name)
    assert set(worst) == set(nc.GRAD_DEV_NARROW)
    for fam, (dev, name) in sorted(worst.items()):
        print("GRAD_DEV_NARROW %s: measured %.3e at %s, table %.3e" % (fam, dev, name, nc.GRAD_DEV_NARROW[fam]))
        assert dev <= nc.GRAD_DEV_NARROW[fam], (fam, dev, name)
        assert 4 * nc.GRAD_DEV_NARROW[fam] < TOL_CAP
