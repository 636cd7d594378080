"""Float64 reference of DistMult written for these tests: scores, the training step with both regularisers,
link-prediction rows.

  ent [E, D], rel [R, D], nothing normalised;  s = sum_j h_j r_j t_j, associated h * (r * t) in head_batch and
  (h * r) * t otherwise (float32 association only);  forward returns s, predict -s.
  A batch holds B positives with K negatives each, negative k of positive i at (k + 1) * B + i.
    sigmoid:   L = -1/2 [ mean_i logsig(p_i) + mean_i sum_k w_ik logsig(-n_ik) ],        w = softmax_k(T n) or 1 / K
    softplus:  L =  1/2 [ mean_i softplus(-p_i) + mean_i sum_k w_ik softplus(n_ik) ]     with nn.Softplus's threshold
               (softplus(x) = x beyond 20): written in the threshold form, so that the tests check that it is
               SigmoidLoss's function to float32 and do not rely on it
  with the weights constants of the backward pass;
    regul_rate:     + regul_rate * (mean(h^2) + mean(t^2) + mean(r^2)) / 3 over the rows as the data loader hands them
                    over: every slot's in normal mode; in head_batch / tail_batch the varying side per slot, the fixed
                    side and the relation once per positive (their first B entries);
    l3_regul_rate:  + l3_regul_rate * (sum |ent|^3 + sum |rel|^3) over the whole tables.

The forward is written in torch and the gradients come from autograd. The same forward evaluated in float32 gives
SCORE_DEV and the cases' own float32 deviation (distmult_cases.py admits a case only if that is small).

GRAD_DEV[family]: the measured worst deviation of the reference implementation's own float32 gradients (the SGD lr 1
table deltas of tests/golden/distmult_g*.npz) from this float64 form, per loss family (SoftplusLoss counts as
SigmoidLoss's), rounded up to two digits; test_distmult_reference_cpu.py measures it again and asserts that it has
not grown. Measured: sigmoid_adv 1.203e-7 (g1, g3, g5; the worst is g3, whose uniform init gives losses near 6),
sigmoid 6.247e-8 (g2, g4, g6).
LOSS_DEV: the worst |recorded float32 loss - float64 loss| / max(1, |float64 loss|) over every recorded step of
distmult_g*.npz (measured 1.099e-7, g3), rounded up likewise.
SCORE_DEV[D]: the worst |float32 - float64| / max(1, |float64|) of this forward evaluated by torch in float32 over the
three modes and both link-prediction sides on score_case(D) (the inputs of the GPU score tests), rounded up to two
digits; pinned to the reference implementation by distmult_p*.npz (its float32 predict is this float32 forward).
None of the three is taken from the kernels.
"""
import numpy as np
import torch

from adv_reference import adam_update, adam_weights, expand_batch  # noqa: F401  (re-exported for the tests)
from rotate_reference import expand_predict  # noqa: F401

TABLES = ("ent_embeddings", "rel_embeddings")
E, R = 37, 3   # the synthetic cases' table sizes

GRAD_DEV = {
    "sigmoid_adv": 1.3e-7,
    "sigmoid": 6.3e-8,
}
LOSS_DEV = 1.1e-7

SCORE_DIMS = (5, 8, 20, 200, 260, 512, 1024)
SCORE_DEV = {5: 1.8e-7, 8: 2.8e-7, 20: 2.6e-7, 200: 3.5e-7, 260: 4.0e-7, 512: 4.4e-7, 1024: 3.2e-7}


def family(cfg):
    return "sigmoid_adv" if cfg.get("adv_temperature") is not None else "sigmoid"


def _broadcast(table, idx, bs):
    """table[idx] for an index that repeats its first bs entries: gathered once and broadcast, as the model gathers the
    fixed side and the relation of a head_batch / tail_batch."""
    rows = table[idx[:bs]]
    return rows.unsqueeze(0).expand(idx.numel() // bs, bs, rows.shape[-1]).reshape(idx.numel(), rows.shape[-1])


def slot_rows(tabs, h, t, r, mode="normal", bs=None):
    """(hv, tv, rv, regul rows) from table tensors of one dtype, the batch in the expanded layout: the [n, D] rows of
    every slot, and the three row sets DistMult.regularization takes its means over (with bs, a head_batch / tail_batch
    holds its fixed side and its relation once per positive)."""
    ent, rel = tabs
    compact = bs is not None and mode != "normal"
    if compact:
        fixed_h, fixed_t = mode == "tail_batch", mode == "head_batch"
        hc = ent[h[:bs]] if fixed_h else ent[h]
        tc = ent[t[:bs]] if fixed_t else ent[t]
        rc = rel[r[:bs]]
        hv = _broadcast(ent, h, bs) if fixed_h else hc
        tv = _broadcast(ent, t, bs) if fixed_t else tc
        return hv, tv, _broadcast(rel, r, bs), (hc, tc, rc)
    hv, tv, rv = ent[h], ent[t], rel[r]
    return hv, tv, rv, (hv, tv, rv)


def _score(hv, tv, rv, mode):
    return (hv * (rv * tv) if mode == "head_batch" else (hv * rv) * tv).sum(-1)


def scores(tables, h, t, r, mode="normal", dtype=torch.float64):
    """The scores s as a numpy array, evaluated by torch in `dtype` (batch in the expanded layout)."""
    tabs = [torch.tensor(np.asarray(x), dtype=dtype) for x in tables]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    with torch.no_grad():
        hv, tv, rv, _ = slot_rows(tabs, hh, tt, rr, mode)
        return _score(hv, tv, rv, mode).numpy()


def loss_value(tabs, h, t, r, bs, cfg, mode="normal"):
    """The step's loss (0-dim tensor) and the scores, in the tables' dtype. cfg: loss ("sigmoid" | "softplus"),
    adv_temperature, regul_rate, l3_regul_rate."""
    hv, tv, rv, (hc, tc, rc) = slot_rows(tabs, h, t, r, mode, bs)
    s = _score(hv, tv, rv, mode)
    p = s[:bs].view(-1, bs).permute(1, 0)   # [B, 1]
    n = s[bs:].view(-1, bs).permute(1, 0)   # [B, K]
    temp = cfg.get("adv_temperature")
    w = torch.softmax(n * temp, -1).detach() if temp is not None else None
    if cfg["loss"] == "sigmoid":
        ls = torch.nn.functional.logsigmoid
        neg = (w * ls(-n)).sum(-1).mean() if w is not None else ls(-n).mean()
        loss = -(ls(p).mean() + neg) / 2
    else:
        sp = torch.nn.Softplus()   # beta 1, threshold 20
        neg = (w * sp(n)).sum(-1).mean() if w is not None else sp(n).mean()
        loss = (sp(-p).mean() + neg) / 2
    regul, l3 = float(cfg.get("regul_rate") or 0.0), float(cfg.get("l3_regul_rate") or 0.0)
    if regul != 0:
        loss = loss + regul * ((hc ** 2).mean() + (tc ** 2).mean() + (rc ** 2).mean()) / 3
    if l3 != 0:
        loss = loss + l3 * ((tabs[0].abs() ** 3).sum() + (tabs[1].abs() ** 3).sum())
    return loss, s


def loss_and_grads(tables, h, t, r, bs, cfg, mode="normal", dtype=torch.float64):
    """(loss, [gradient of ent, of rel as float64 arrays], aux) of one batch in the expanded layout, evaluated by torch
    in `dtype`. aux: gmax (largest |gradient| element), s (the scores)."""
    tabs = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in tables]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    loss, s = loss_value(tabs, hh, tt, rr, bs, cfg, mode)
    loss.backward()
    grads = [x.grad.double().numpy().copy() if x.grad is not None else np.zeros(tuple(x.shape)) for x in tabs]
    aux = {"gmax": max(float(np.abs(g).max()) for g in grads), "s": s.detach().double().numpy().copy()}
    return float(loss.detach()), grads, aux


def grad_bound(fam, gmax):
    """The project's parity bound of a gradient cell (rotate_reference.grad_bound): four float32 ulps of the largest
    gradient (at least of 1), or four times the reference implementation's own float32 deviation, capped at 1e-5."""
    return min(1e-5, max(4 * 2.0 ** -23 * max(1.0, gmax), 4 * GRAD_DEV[fam]))


def score_tol(D):
    """rotate_reference.score_tol: a score cell, relative to max(1, |score|)."""
    return min(1e-5, max(4 * 2.0 ** -23, 4 * SCORE_DEV[D]))


def loss_tol():
    """A loss value, relative to max(1, |L|): four times the reference's own float32 deviation, capped at 1e-5."""
    return min(1e-5, 4 * LOSS_DEV)


def loss_close(loss, want):
    return abs(loss - want) <= loss_tol() * max(1.0, abs(want))


def lp_scores(tables, anchor, r, side, dtype=torch.float64):
    """[E] predict values (-s) of every entity as the missing side of one query: side 0 head prediction (anchor = the
    tail, the head_batch form), side 1 tail prediction (anchor = the head)."""
    n = np.asarray(tables[0]).shape[0]
    cand = np.arange(n, dtype=np.int64)
    fixed = np.full(n, anchor, dtype=np.int64)
    rr = np.full(n, r, dtype=np.int64)
    if side == 0:
        return -scores(tables, cand, fixed, rr, "head_batch", dtype)
    return -scores(tables, fixed, cand, rr, "tail_batch", dtype)


# ---------------------------------------------------------------------------------------- fixtures
def golden_cfg(z):
    """The configuration dict of a tests/golden/distmult_g*.npz / distmult_a*.npz file."""
    def opt(key):
        x = float(z[key])
        return None if np.isnan(x) else x
    return {"model": "DistMult", "loss": str(z["loss"]), "adv_temperature": opt("adv_temperature"),
            "regul_rate": float(z["regul_rate"]), "l3_regul_rate": float(z["l3_regul_rate"]),
            "model_margin": opt("model_margin"), "epsilon": opt("epsilon"), "sampling": str(z["sampling"]),
            "dim": int(z["dim"]), "batch_size": int(z["batch_size"]), "neg_ent": int(z["neg_ent"]),
            "torch_seed": int(z["torch_seed"])}


def golden_tables(z, tag):
    """(ent, rel) arrays stored under `tag` (or untagged) in a golden file."""
    pre = tag + "_" if tag else ""
    return tuple(z[pre + k] for k in TABLES)


def golden_step(z, cfg, s):
    """Step s's batch of a golden run in the expanded layout, and its mode."""
    mode = str(z["modes"][s])
    return expand_batch(z["b%d_h" % s], z["b%d_t" % s], z["b%d_r" % s], mode, cfg["batch_size"]), mode


# ---------------------------------------------------------------------------------------- score cases
def table_scale(D):
    """a of uniform(+-a) tables whose scores have a standard deviation near 1.5: a = sqrt(3) (1.5 / sqrt(D))^(1/3)."""
    return float(np.sqrt(3.0) * (1.5 / np.sqrt(D)) ** (1.0 / 3.0))


def score_case(D):
    """Tables (E = 37, R = 3, uniform(+-table_scale(D))) and the three modes' batches of the score tests at dim D
    ({mode: (h, t, r) as predict takes them})."""
    rng = np.random.default_rng(9100 + D)
    a = table_scale(D)
    tabs = [rng.uniform(-a, a, size=(E, D)).astype(np.float32), rng.uniform(-a, a, size=(R, D)).astype(np.float32)]
    n = 41
    h, t, r = rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)
    batches = {"normal": (h, t, r), "head_batch": (rng.integers(0, E, n), t[:1], r[:1]),
               "tail_batch": (h[:1], rng.integers(0, E, n), r[:1])}
    return tabs, batches


def measure_score_dev(D):
    """Worst relative deviation of the float32 torch forward from float64 over score_case(D)."""
    worst = 0.0
    tabs, batches = score_case(D)
    for mode, (h, t, r) in batches.items():
        hh, tt, rr = expand_predict(h, t, r, mode)
        ref = scores(tabs, hh, tt, rr, mode, torch.float64)
        got = scores(tabs, hh, tt, rr, mode, torch.float32).astype(np.float64)
        worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
        for side in (0, 1):   # the link-prediction rows of the same tables
            ref = lp_scores(tabs, int(h[0]), int(r[0]), side)
            got = lp_scores(tabs, int(h[0]), int(r[0]), side, torch.float32).astype(np.float64)
            worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
    return worst


def measure_grad_dev(z):
    """(worst |reference float32 gradient - float64 gradient|, worst relative loss deviation) over the steps of one
    distmult_g*.npz (the SGD lr 1 table deltas and the recorded losses against this form at the tables before each
    step)."""
    cfg = golden_cfg(z)
    worst, lworst = 0.0, 0.0
    for s in range(int(z["steps"])):
        (h, t, r), mode = golden_step(z, cfg, s)
        before, after = golden_tables(z, "s%d" % s), golden_tables(z, "s%d" % (s + 1))
        loss, grads, _ = loss_and_grads(before, h, t, r, cfg["batch_size"], cfg, mode)
        lworst = max(lworst, abs(float(z["losses"][s]) - loss) / max(1.0, abs(loss)))
        for b, a, g in zip(before, after, grads):
            worst = max(worst, float(np.abs((b.astype(np.float64) - a.astype(np.float64)) - g).max()))
    return worst, lworst
