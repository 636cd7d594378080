"""The cases of tests/test_gpu_wide.py (TransE and TransH single models at dims 516..1024, float4 rows with three and
four chunks per lane), shared with tests/test_wide_reference_cpu.py, which checks their input conditions and measures
the two deviation tables below on the CPU.

Tables are uniform(-1, 1) * scale over E = 70 entities and R = 3 relations, so rows collide constantly; batches are
given explicitly as B = 11 / K = 3 and B = 37 / K = 7 (k_step_adv also K = 70: more scores than lanes). Entity 69 and
relation 2 are never drawn by the plain-step and Adam batches (their rows must stay bit-identical).

The wide dims: 516 (third chunk with one live lane), 768 (three chunks exactly full), 772 (fourth chunk with one live
lane), 1024.

Tolerances are the project's rules (test_gpu_lp_values.py, test_gpu_adv.py) with the deviation tables extended to
these dims by measurement on the CPU, never from the kernels:
  scores    tol(D) = min(1e-5, max(4 * 2^-23, 4 * ORACLE_DEV_WIDE[D])) relative to max(1, ref64)
  gradients min(1e-5, max(4 * 2^-23 * max(1, |g|max), 4 * GRAD_DEV_WIDE[family]))
"""
import numpy as np
import torch

import adv_cases
import adv_reference as ar

E, R = 70, 3
FREE_ENT, FREE_REL = E - 1, R - 1   # never in a plain-step or Adam batch
ONCE_ENT = E - 2                    # Adam: in step 1 only
WIDE_DIMS = (516, 768, 772, 1024)

# Worst |oracle.score - lp_scores64| / max(1, ref64) per dim, measured exactly as lp_reference.ORACLE_DEV is
# (test_lp_reference_cpu._deviation: model x p x norm_flag on uniform(-1, 1) tables), rounded up to three digits.
ORACLE_DEV_WIDE = {516: 1.61e-6, 768: 1.93e-6, 772: 1.79e-6, 1024: 2.25e-6}

# Worst |float32 torch autograd gradient - float64 gradient| of adv_reference's forward on the GPU cases' own inputs,
# per family (grad_dev below), rounded up to two digits.
GRAD_DEV_WIDE = {
    "plain_TransE": 3.3e-7,
    "plain_TransH": 3.4e-7,
    "sigmoid_adv": 1.1e-6,   # p = 1 on raw rows: distances of 400 to 800, whose float32 ulp the sigmoid passes on
    "sigmoid": 4.4e-10,
    "margin_adv": 7.6e-9,
    "margin_model": 1.6e-10,
}

TOL_FLOOR, TOL_CAP = 4 * 2.0 ** -23, 1e-5


def score_tol(D):
    return min(TOL_CAP, max(TOL_FLOOR, 4 * ORACLE_DEV_WIDE[D]))


def family(cfg):
    if cfg.get("plain"):
        return "plain_" + cfg["model"]
    return ar.family(cfg)


def grad_tol(gmax, cfg):
    return min(TOL_CAP, max(TOL_FLOOR * max(1.0, gmax), 4 * GRAD_DEV_WIDE[family(cfg)]))


# ---------------------------------------------------------------------------------------- scores
def _normalize(x):
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)


def scores64(model, p, nf, tabs, h, t, r):
    """float64 distances of the slots (h, t, r) from float32 tables (ent, rel, norm_vector or None)."""
    ent, rel = (np.asarray(x, dtype=np.float64) for x in tabs[:2])
    hv, tv, rv = ent[h], ent[t], rel[r]
    if model == "TransH":
        w = _normalize(np.asarray(tabs[2], dtype=np.float64)[r])
        hv = hv - (hv * w).sum(-1, keepdims=True) * w
        tv = tv - (tv * w).sum(-1, keepdims=True) * w
    if nf:
        hv, tv, rv = _normalize(hv), _normalize(tv), _normalize(rv)
    v = (hv + rv) - tv
    return np.abs(v).sum(-1) if p == 1 else np.sqrt((v * v).sum(-1))


def score_case(model, D, p, nf):
    """Tables and the three modes' batches (as predict takes them) of the score tests."""
    rng = np.random.default_rng(8000 + 10 * D + 4 * (model == "TransH") + 2 * p + int(nf))
    tabs = adv_cases.make_tables(rng, D, 1.0, ent=E, rel=R, transh=model == "TransH")
    n = 41
    h, t, r = rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)
    batches = {"normal": (h, t, r), "head_batch": (rng.integers(0, E, n), t[:1], r[:1]),
               "tail_batch": (h[:1], rng.integers(0, E, n), r[:1])}
    return tabs, batches


def expand_predict(h, t, r):
    h, t, r = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (h, t, r))
    n = max(h.size, t.size)
    return np.resize(h, n), np.resize(t, n), np.resize(r, n)


# ---------------------------------------------------------------------------------------- the plain step
# loss margins that leave between 20 % and 80 % of the pairs active: of the size of the spread of p - n, not of the
# distances themselves (which concentrate at these dims)
PLAIN_MARGIN = {(1, True): 0.1, (1, False): 4.0, (2, True): 0.01, (2, False): 0.1}


def _plain_cases():
    out = []
    for D in WIDE_DIMS:
        for model in ("TransE", "TransH"):
            for p in (1, 2):
                for opt in ("sgd", "adagrad"):
                    nf = (opt == "sgd") == (model == "TransE")
                    # p = 1 with normalised rows keeps to the small batch: |v| components are ~ 1 / sqrt(D) there, and
                    # none may lie within 1e-6 of zero
                    small = nf if p == 1 else not nf
                    B, K = (11, 3) if small else (37, 7)
                    name = "%s-d%d-p%d-%s-%s-b%d" % (model, D, p, "nf" if nf else "raw", opt, B)
                    out.append((name, model, D, B, K, nf, p, opt, PLAIN_MARGIN[(p, nf)]))
    return out


PLAIN_CASES = _plain_cases()
# seeds under which the input conditions hold (test_wide_reference_cpu.py); every other case uses seed 1
PLAIN_SEEDS = {"TransH-d768-p1-raw-sgd-b37": 4, "TransE-d772-p1-nf-sgd-b11": 2}


def plain_cfg(case):
    name, model, D, B, K, nf, p, opt, margin = case
    return {"model": model, "loss": "margin", "adv_temperature": None, "loss_margin": margin, "p_norm": p,
            "norm_flag": nf, "model_margin": None, "dim": D, "batch_size": B, "neg_ent": K, "plain": True}


def make_plain_batch(rng, B, K):
    """The expanded batch (h, t, r of length B * (K + 1)): every negative replaces the tail or the head of its
    positive, then the planted slots (B >= 11): positive 0 a self-loop; negative 0 of positive 1 equal to its
    positive; negative 0 of positive 2 differing in all three ids; positive 3's head = the corrupted tail of negative
    0 of positive 4 (atomics of two lane groups meeting on one row)."""
    h = rng.integers(0, FREE_ENT, size=B)
    t = rng.integers(0, FREE_ENT, size=B)
    r = rng.integers(0, FREE_REL, size=B)
    n = B * K
    hh, tt, rr = np.tile(h, K), np.tile(t, K), np.tile(r, K)
    new_e = rng.integers(0, FREE_ENT, size=n)
    tails = rng.random(n) < 0.5
    tt = np.where(tails, new_e, tt)
    hh = np.where(~tails, new_e, hh)
    bh, bt, br = (np.concatenate(x).astype(np.int64) for x in ((h, hh), (t, tt), (r, rr)))
    bt[0] = bh[0]
    for k in range(K):
        o = (k + 1) * B
        if bh[o] != bh[0]:
            bt[o] = bt[0]   # a head corruption keeps the self-loop's tail
    o = B + 1
    bh[o], bt[o], br[o] = bh[1], bt[1], br[1]
    o = B + 2
    bh[o], bt[o], br[o] = (bh[2] + 1) % FREE_ENT, (bt[2] + 1) % FREE_ENT, 1 - br[2]
    o = B + 4
    bh[o], bt[o], br[o] = bh[4], bh[3], br[4]
    return bh, bt, br


def planted(bh, bt, br, B, K):
    """Which planted slot kinds a plain batch holds."""
    hn, tn, rn = (x[B:].reshape(K, B) for x in (bh, bt, br))
    hp, tp, rp = bh[:B], bt[:B], br[:B]
    ents, counts = np.unique(np.concatenate([bh, bt]), return_counts=True)
    return {"self_loop": bool((hp == tp).any()),
            "neg_equals_pos": bool(((hn == hp) & (tn == tp) & (rn == rp)).any()),
            "all_three_differ": bool(((hn != hp) & (tn != tp) & (rn != rp)).any()),
            "shared_entity": bool(((tn[0, 4] == hp[3]) and counts.max() > 2)),
            "free_entity": FREE_ENT not in ents, "free_relation": FREE_REL not in br}


def build_plain(case):
    """(tables, (h, t, r) expanded, cfg) of a plain-step case."""
    name, model, D, B, K, nf, p, opt, margin = case
    rng = np.random.default_rng(5000 + PLAIN_SEEDS.get(name, 1))
    tabs = adv_cases.make_tables(rng, D, 1.0, ent=E, rel=R, transh=model == "TransH")
    return tabs, make_plain_batch(rng, B, K), plain_cfg(case)


def as_batch(hrt):
    h, t, r = hrt
    return {"batch_h": h, "batch_t": t, "batch_r": r, "batch_y": np.zeros(len(h), dtype=np.float32), "mode": "normal"}


# ---------------------------------------------------------------------------------------- the weighted step
# adv_cases.GRAD_CASES' four families and its stability case at the wide dims (TransE; the tuple layout is adv_cases'):
# id, D, B, K, mode, norm_flag, p, loss, adv_temperature, loss margin, model margin, table scale, seed.
# p = 1 keeps to B = 11 / K = 3 and raw rows (see _plain_cases); its model margin is the size of the distances
# (0.77 D: the mean of |u1 + u2 - u3|, u uniform(-1, 1), is 0.77), its temperature of the size of the inverse of their
# spread (about 0.55 sqrt(D)), so that the weights vary without being one-hot.
def _adv_cases():
    out = []
    for i, D in enumerate(WIDE_DIMS):
        out += [
            ("d%d-sigmoid-k70-tail" % D, D, 11, 70, "tail_batch", True, 2, "sigmoid", None, None, 6.0, 1.0, 1),
            ("d%d-sigmoid-adv-p1" % D, D, 11, 3, "normal", False, 1, "sigmoid", 0.1, None, round(0.77 * D), 1.0, 1),
            ("d%d-margin-adv-head" % D, D, 37, 7, "head_batch", False, 2, "margin", 2.0, 0.1, None, 1.0, 1),
            ("d%d-margin-model" % D, D, 37, 7, "normal", True, 2, "margin", None, 0.01, 5.0, 1.0, 1),
        ]
    return out


ADV_CASES = _adv_cases()
# distances around sqrt(D) (23 to 32) at temperature 40 on unnormalised rows, K = 70
STABILITY_CASES = [("d%d-stability" % D, D, 11, 70, "normal", False, 2, "sigmoid", 40.0, None, 6.0, 1.0, 1)
                   for D in WIDE_DIMS]
ADV_SEEDS = {}


def build_adv(case):
    """(tables, batch dict, cfg) of a weighted case (adv_cases.build over E = 70, R = 3)."""
    name, D, B, K, mode, nf, p, loss, temp, lmargin, gamma, scale, seed = case
    rng = np.random.default_rng(6000 + ADV_SEEDS.get(name, seed))
    return (adv_cases.make_tables(rng, D, scale, ent=E, rel=R), adv_cases.make_batch(rng, B, K, mode, ent=E, rel=R),
            adv_cases.case_cfg(case))


def expanded(batch, bs):
    return ar.expand_batch(batch["batch_h"], batch["batch_t"], batch["batch_r"], batch["mode"], bs)


# ---------------------------------------------------------------------------------------- Adam
# three steps from a given state; entity 68 appears in step 1 only (as a corrupted tail), entity 69 never
# id, model, D, B, K, norm_flag, p, loss, adv_temperature, loss margin, model margin, lr, first step, seed
ADAM_CASES = [c for D in WIDE_DIMS for c in (
    ("adam-transe-d%d" % D, "TransE", D, 11, 3, True, 2, "sigmoid", 1.0, None, 6.0, 1e-3, 5, 1),
    ("adam-transh-d%d" % D, "TransH", D, 37, 7, True, 2, "margin", None, 0.01, None, 1e-3, 0, 1),
)]
ADAM_STEPS = 3


def build_adam(case):
    """(tables, [batch dict per step], cfg, (m0, v0) per table, lr, steps already done)."""
    name, model, D, B, K, nf, p, loss, temp, lmargin, gamma, lr, step0, seed = case
    rng = np.random.default_rng(7000 + seed)
    tabs = adv_cases.make_tables(rng, D, 1.0, ent=E, rel=R, transh=model == "TransH")
    batches = [as_batch(make_plain_batch(rng, B, K)) for _ in range(ADAM_STEPS)]
    for b in batches:   # entity 68 only where planted below
        for key in ("batch_h", "batch_t"):
            b[key][b[key] == ONCE_ENT] = 0
    b0 = batches[0]
    for i in range(5, 11):   # negative 0 of positives 5 to 10: corrupted tail = entity 68 (a margin loss leaves some
                             # of them without a gradient)
        o = B + i
        b0["batch_h"][o], b0["batch_t"][o], b0["batch_r"][o] = b0["batch_h"][i], ONCE_ENT, b0["batch_r"][i]
    m0, v0 = [], []
    for x in tabs:
        if x is None:
            m0.append(None); v0.append(None)
            continue
        m = (0.01 * rng.uniform(-1, 1, size=x.shape)).astype(np.float32)
        v = (1e-5 * rng.uniform(0, 1, size=x.shape)).astype(np.float32)
        if x.shape[0] == E:
            m[ONCE_ENT:] = 0
            v[ONCE_ENT:] = 0
        m0.append(m); v0.append(v)
    cfg = {"model": model, "loss": loss, "adv_temperature": temp, "loss_margin": lmargin, "p_norm": p,
           "norm_flag": nf, "model_margin": gamma, "dim": D, "batch_size": B, "neg_ent": K,
           "plain": loss == "margin" and temp is None and gamma is None}
    return tabs, batches, cfg, (m0, v0), lr, step0


# ---------------------------------------------------------------------------------------- conditions, deviations
def conditions(tabs, h, t, r, bs, cfg):
    """The float64 loss, gradients and input conditions of a batch: aux of adv_reference.loss_and_grads plus `active`,
    the share of (positive, negative) pairs on the sloped side of a margin loss's hinge (nan for the sigmoid loss)."""
    loss, grads, aux = ar.loss_and_grads(tabs, h, t, r, bs, cfg)
    aux["active"] = float("nan")
    if cfg["loss"] == "margin":
        d = aux["d"]
        s = cfg["model_margin"] - d if cfg.get("model_margin") is not None else d
        pos, neg = s[:bs][None, :], s[bs:].reshape(-1, bs)
        aux["active"] = float((pos - neg + cfg["loss_margin"] > 0).mean())
    return loss, grads, aux


def grads32(tabs, h, t, r, bs, cfg):
    """The gradients of adv_reference's forward evaluated in float32 by torch autograd (float64 arrays). On one
    thread: the order in which the row gradients of a table are summed, and so the float32 result, is then fixed."""
    tt = [torch.tensor(np.asarray(x, dtype=np.float32), requires_grad=True) for x in tabs if x is not None]
    hh, t_, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        loss, _ = ar.loss_value(tt, hh, t_, rr, bs, cfg)
        loss.backward()
    finally:
        torch.set_num_threads(threads)
    return [x.grad.numpy().astype(np.float64) if x.grad is not None else np.zeros(tuple(x.shape)) for x in tt]


def grad_dev(tabs, h, t, r, bs, cfg):
    """Worst |float32 gradient - float64 gradient| over every table of one batch."""
    _, g64, _ = ar.loss_and_grads(tabs, h, t, r, bs, cfg)
    g32 = grads32(tabs, h, t, r, bs, cfg)
    return max(float(np.abs(a - b).max()) for a, b in zip(g32, g64))


def gradient_inputs():
    """Every (family, name, tables, (h, t, r) expanded, bs, cfg) the GPU gradient and Adam tests run."""
    for case in PLAIN_CASES:
        tabs, hrt, cfg = build_plain(case)
        yield family(cfg), case[0], tabs, hrt, cfg["batch_size"], cfg
    for case in ADV_CASES + STABILITY_CASES:
        tabs, batch, cfg = build_adv(case)
        yield family(cfg), case[0], tabs, expanded(batch, cfg["batch_size"]), cfg["batch_size"], cfg
    for case in ADAM_CASES:
        tabs, batches, cfg, _, _, _ = build_adam(case)
        for s, b in enumerate(batches):
            yield family(cfg), "%s-step%d" % (case[0], s), tabs, expanded(b, cfg["batch_size"]), cfg["batch_size"], cfg


# ---------------------------------------------------------------------------------------- link prediction
# Tester.run_link_prediction on kg_small: model, dim, p_norm, norm_flag, table seed (seeds under which at most 2 % of
# the queries hold a near tie: test_wide_reference_cpu.py; of nine seeds tried for TransE, six met it)
LP_CASES = [("TransE", 1024, 1, False, 45), ("TransH", 772, 2, False, 42)]


def lp_tables(case, ent_tot, rel_tot):
    """(ent, rel, norm_vector or None): uniform(-1, 1) rows, each entity row scaled by uniform(0.5, 4). Rows
    of one scale give distances that concentrate at these dims (a spread of 2 % of their size: with 500 candidates a
    fifth of the queries would hold a near tie); the row scales spread them over a factor of about five."""
    model, D, p, nf, seed = case
    rng = np.random.default_rng(9000 + seed)
    ent = rng.uniform(-1, 1, size=(ent_tot, D)) * rng.uniform(0.5, 4, size=(ent_tot, 1))
    rel = rng.uniform(-1, 1, size=(rel_tot, D))
    nv = rng.uniform(-1, 1, size=(rel_tot, D)).astype(np.float32) if model == "TransH" else None
    return ent.astype(np.float32), rel.astype(np.float32), nv


def lp_rows64(case, tabs, h, t, r):
    """(head rows, tail rows) float64 [n][E]: every entity scored as the missing head / tail of each query."""
    from lp_reference import lp_scores64
    model, D, p, nf, _ = case
    ent, rel, nv = tabs
    rows_h = np.stack([lp_scores64(model, p, nf, ent, rel, nv, int(t[i]), int(r[i]), 0) for i in range(len(h))])
    rows_t = np.stack([lp_scores64(model, p, nf, ent, rel, nv, int(h[i]), int(r[i]), 1) for i in range(len(h))])
    return rows_h, rows_t


def ranks_from_rows(rows_h, rows_t, h, t, r, known):
    """(raw head, filtered head, raw tail, filtered tail) ranks of Test.h:118-359 from entity-order score rows, counted
    from 0 as the oracle and Tester.last_ranks count them: the candidates scoring strictly below the truth (filtered:
    those that are not known triples). `known` is a set of (h, t, r)."""
    n = len(h)
    out = [np.zeros(n, dtype=np.int64) for _ in range(4)]
    for i in range(n):
        for side, rows, truth in ((0, rows_h, int(h[i])), (1, rows_t, int(t[i]))):
            s = rows[i]
            below = np.nonzero(s < s[truth])[0]
            below = below[below != truth]
            if side == 0:
                filt = sum((int(j), int(t[i]), int(r[i])) not in known for j in below)
            else:
                filt = sum((int(h[i]), int(j), int(r[i])) not in known for j in below)
            out[2 * side][i] = len(below)
            out[2 * side + 1][i] = filt
    return out


def lp_near_ties(case, rows_h, rows_t, h, t):
    """[2][n] whether query n's side holds a candidate other than the truth within score_tol(D), relative to
    max(1, |truth score|), of the truth's float64 score: the band inside which a GPU score within its tolerance may
    order the two differently."""
    band = score_tol(case[1])
    out = np.zeros((2, len(h)), dtype=bool)
    for i in range(len(h)):
        for side, rows, truth in ((0, rows_h, int(h[i])), (1, rows_t, int(t[i]))):
            s = rows[i]
            out[side, i] = (np.abs(s - s[truth]) <= band * max(1.0, abs(s[truth]))).sum() > 1
    return out
