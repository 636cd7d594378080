"""Float64 reference of ComplEx written for these tests: scores, the training step with the regulariser,
link-prediction rows.

  ent_re, ent_im [E, D], rel_re, rel_im [R, D], nothing normalised;
  s = sum_j h_re t_re r_re + h_im t_im r_re + h_re t_im r_im - h_im t_re r_im;  forward returns s, predict -s.
  A batch holds B positives with K negatives each, negative k of positive i at (k + 1) * B + i; training batches are
  normal-mode only (the model's forward ignores the batch mode), predict broadcasts in head_batch / tail_batch.
    sigmoid:   L = -1/2 [ mean_i logsig(p_i) + mean_i sum_k w_ik logsig(-n_ik) ],        w = softmax_k(T n) or 1 / K
    softplus:  L =  1/2 [ mean_i softplus(-p_i) + mean_i sum_k w_ik softplus(n_ik) ]     with nn.Softplus's threshold
               (softplus(x) = x beyond 20): written in the threshold form
  with the weights constants of the backward pass;
    regul_rate:  + regul_rate * (mean h_re^2 + mean h_im^2 + mean t_re^2 + mean t_im^2 + mean r_re^2 + mean r_im^2) / 6
                 over every slot's rows.
  `variant` evaluates a deliberately wrong model, for the admission conditions of complex_cases.py only: "flip" flips
  the sign of the h_im t_re r_im term, "no_im" zeroes both im tables.

The forward is written in torch and the gradients come from autograd. The same forward evaluated in float32 gives the
three deviations below; none of them is taken from the kernels. Command that measures them again (and asserts that none
has grown):  python -m pytest tests/test_complex_reference_cpu.py -k "dev_is_measured" -s

GRAD_DEV[family]: the worst |float32 gradient - float64 gradient| of this forward evaluated by torch in float32 over
every case of complex_cases.py (gradient, threshold, Adagrad, many-relations and every Adam step) and over every
recorded step of tests/golden/complex_g*.npz (there the float32 gradient is the reference implementation's own SGD lr 1
table delta), per loss family (SoftplusLoss counts as SigmoidLoss's), rounded up to two digits. Measured: sigmoid_adv
9.062e-8 (d20-k70-sig-adv-reg), sigmoid 6.950e-8 (d20-soft-threshold); the fixtures' worst is 4.086e-8 (complex_g2).
LOSS_DEV: the worst |float32 loss - float64 loss| / max(1, |float64 loss|) over the same runs (measured 9.462e-8,
d12-many-rel-reg; the fixtures' worst is 6.212e-8, complex_g4), rounded up likewise.
SCORE_DEV[D]: the worst |float32 - float64| / max(1, |float64|) of this forward over the three modes and both
link-prediction sides on score_case(D) (the inputs of the GPU score tests), rounded up to two digits; pinned to the
reference implementation by complex_p*.npz (its float32 predict is this float32 forward).
"""
import numpy as np
import torch

from adv_reference import adam_update, adam_weights  # noqa: F401  (re-exported for the tests)
from rotate_reference import expand_predict  # noqa: F401

# the four tables in the reference's construction order (the tests address the model's tables by these names)
TABLES = ("ent_re_embeddings", "ent_im_embeddings", "rel_re_embeddings", "rel_im_embeddings")
E, R = 37, 3   # the synthetic cases' table sizes

GRAD_DEV = {
    "sigmoid_adv": 9.1e-8,
    "sigmoid": 7.0e-8,
}
LOSS_DEV = 9.5e-8

SCORE_DIMS = (1, 2, 3, 5, 8, 20, 200, 260, 512, 516, 1024)
SCORE_DEV = {1: 2.2e-7, 2: 2.0e-7, 3: 2.1e-7, 5: 3.0e-7, 8: 3.2e-7, 20: 3.8e-7, 200: 4.6e-7, 260: 5.0e-7, 512: 4.1e-7,
             516: 5.5e-7, 1024: 5.9e-7}


def family(cfg):
    return "sigmoid_adv" if cfg.get("adv_temperature") is not None else "sigmoid"


def _score(tabs, h, t, r, variant=None):
    ent_re, ent_im, rel_re, rel_im = tabs
    if variant == "no_im":
        ent_im, rel_im = ent_im * 0, rel_im * 0
    h_re, h_im, t_re, t_im, r_re, r_im = ent_re[h], ent_im[h], ent_re[t], ent_im[t], rel_re[r], rel_im[r]
    sign = 1.0 if variant == "flip" else -1.0
    s = torch.sum(h_re * t_re * r_re + h_im * t_im * r_re + h_re * t_im * r_im + sign * (h_im * t_re * r_im), -1)
    return s, (h_re, h_im, t_re, t_im, r_re, r_im)


def scores(tables, h, t, r, dtype=torch.float64):
    """The scores s as a numpy array, evaluated by torch in `dtype` (h, t, r of equal length)."""
    tabs = [torch.tensor(np.asarray(x), dtype=dtype) for x in tables]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    with torch.no_grad():
        return _score(tabs, hh, tt, rr)[0].numpy()


def loss_value(tabs, h, t, r, bs, cfg, variant=None):
    """The step's loss (0-dim tensor) and the scores, in the tables' dtype. cfg: loss ("sigmoid" | "softplus"),
    adv_temperature, regul_rate."""
    s, rows = _score(tabs, h, t, r, variant)
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
    regul = float(cfg.get("regul_rate") or 0.0)
    if regul != 0:
        loss = loss + regul * sum((x ** 2).mean() for x in rows) / 6
    return loss, s


def loss_and_grads(tables, h, t, r, bs, cfg, dtype=torch.float64, variant=None):
    """(loss, [gradients of the four tables in TABLES' order as float64 arrays], aux) of one normal-mode batch,
    evaluated by torch in `dtype`. aux: gmax (largest |gradient| element), s (the scores)."""
    tabs = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in tables]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    loss, s = loss_value(tabs, hh, tt, rr, bs, cfg, variant)
    loss.backward()
    grads = [x.grad.double().numpy().copy() if x.grad is not None else np.zeros(tuple(x.shape)) for x in tabs]
    aux = {"gmax": max(float(np.abs(g).max()) for g in grads), "s": s.detach().double().numpy().copy()}
    return float(loss.detach()), grads, aux


def grad_bound(fam, gmax):
    """The project's parity bound of a gradient cell (distmult_reference.grad_bound): four float32 ulps of the largest
    gradient (at least of 1), or four times the reference formulas' own float32 deviation, capped at 1e-5."""
    return min(1e-5, max(4 * 2.0 ** -23 * max(1.0, gmax), 4 * GRAD_DEV[fam]))


def score_tol(D):
    """distmult_reference.score_tol: a score cell, relative to max(1, |score|)."""
    return min(1e-5, max(4 * 2.0 ** -23, 4 * SCORE_DEV[D]))


def loss_tol():
    """A loss value, relative to max(1, |L|): four times the reference's own float32 deviation, capped at 1e-5."""
    return min(1e-5, 4 * LOSS_DEV)


def loss_close(loss, want):
    return abs(loss - want) <= loss_tol() * max(1.0, abs(want))


def lp_scores(tables, anchor, r, side, dtype=torch.float64):
    """[E] predict values (-s) of every entity as the missing side of one query: side 0 head prediction (anchor = the
    tail), side 1 tail prediction (anchor = the head)."""
    n = np.asarray(tables[0]).shape[0]
    cand = np.arange(n, dtype=np.int64)
    fixed = np.full(n, anchor, dtype=np.int64)
    rr = np.full(n, r, dtype=np.int64)
    if side == 0:
        return -scores(tables, cand, fixed, rr, dtype)
    return -scores(tables, fixed, cand, rr, dtype)


# ---------------------------------------------------------------------------------------- fixtures
def golden_cfg(z):
    """The configuration dict of a tests/golden/complex_g*.npz / complex_a*.npz file."""
    temp = float(z["adv_temperature"])
    return {"model": "ComplEx", "loss": str(z["loss"]), "adv_temperature": None if np.isnan(temp) else temp,
            "regul_rate": float(z["regul_rate"]), "sampling": str(z["sampling"]), "neg_rel": int(z["neg_rel"]),
            "dim": int(z["dim"]), "batch_size": int(z["batch_size"]), "neg_ent": int(z["neg_ent"]),
            "torch_seed": int(z["torch_seed"])}


def golden_tables(z, tag):
    """The four arrays stored under `tag` (or untagged) in a golden file, in TABLES' order."""
    pre = tag + "_" if tag else ""
    return tuple(z[pre + k] for k in TABLES)


def golden_step(z, s):
    """Step s's batch of a golden run (normal mode: the arrays as recorded)."""
    assert str(z["modes"][s]) == "normal"
    return tuple(np.asarray(z["b%d_%s" % (s, k)], dtype=np.int64) for k in "htr")


# ---------------------------------------------------------------------------------------- score cases
def table_scale(D):
    """a of uniform(+-a) tables whose scores have a standard deviation near 1.5: s sums four DistMult-like terms, so
    sd(s) = 2 sqrt(D) (a^2 / 3)^(3/2) and a = sqrt(3) (0.75 / sqrt(D))^(1/3)."""
    return float(np.sqrt(3.0) * (0.75 / np.sqrt(D)) ** (1.0 / 3.0))


def make_tables(rng, D, ent=E, rel=R):
    a = table_scale(D)
    return [rng.uniform(-a, a, size=(rows, D)).astype(np.float32) for rows in (ent, ent, rel, rel)]


def score_case(D):
    """Tables (E = 37, R = 3, uniform(+-table_scale(D))) and the three modes' batches of the score tests at dim D
    ({mode: (h, t, r) as predict takes them})."""
    rng = np.random.default_rng(9300 + D)
    tabs = make_tables(rng, D)
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
        ref = scores(tabs, hh, tt, rr, torch.float64)
        got = scores(tabs, hh, tt, rr, torch.float32).astype(np.float64)
        worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
        for side in (0, 1):   # the link-prediction rows of the same tables
            ref = lp_scores(tabs, int(h[0]), int(r[0]), side)
            got = lp_scores(tabs, int(h[0]), int(r[0]), side, torch.float32).astype(np.float64)
            worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
    return worst


def measure_case_dev(tabs, hrt, cfg):
    """(worst |float32 gradient - float64 gradient|, relative loss deviation) of torch's float32 evaluation of one
    batch."""
    bs = cfg["batch_size"]
    l64, g64, _ = loss_and_grads(tabs, *hrt, bs, cfg)
    l32, g32, _ = loss_and_grads(tabs, *hrt, bs, cfg, dtype=torch.float32)
    return max(float(np.abs(a - b).max()) for a, b in zip(g32, g64)), abs(l32 - l64) / max(1.0, abs(l64))


def measure_golden_dev(z):
    """(worst |reference float32 gradient - float64 gradient|, worst relative loss deviation) over the steps of one
    complex_g*.npz (the SGD lr 1 table deltas and the recorded losses against this form at the tables before each
    step)."""
    cfg = golden_cfg(z)
    worst, lworst = 0.0, 0.0
    for s in range(int(z["steps"])):
        h, t, r = golden_step(z, s)
        before, after = golden_tables(z, "s%d" % s), golden_tables(z, "s%d" % (s + 1))
        loss, grads, _ = loss_and_grads(before, h, t, r, cfg["batch_size"], cfg)
        lworst = max(lworst, abs(float(z["losses"][s]) - loss) / max(1.0, abs(loss)))
        for b, a, g in zip(before, after, grads):
            worst = max(worst, float(np.abs((b.astype(np.float64) - a.astype(np.float64)) - g).max()))
    return worst, lworst
