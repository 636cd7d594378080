"""Float64 reference of RotatE written for these tests: distances, the weighted training step, link-prediction rows.

  An entity row holds 2 * dim floats, re[0:dim] | im[dim:2 dim]; a relation row dim phases. q = float32(
  rel_embedding_range / pi) (phase_div: a Python double divided by the float32 pi tensor, as the reference forms it);
  phi = r / q, c = cos(phi), s = sin(phi);  v = h o (c + i s) - t  (head_batch: conj(c + i s) o t - h);
  d = sum_j sqrt(v_re[j]^2 + v_im[j]^2);  the score handed to the loss is gamma - d;  predict returns d - gamma.
  A batch holds B positives with K negatives each, negative k of positive i at (k + 1) * B + i.
    sigmoid:  L = -1/2 [ mean_i logsig(p_i) + mean_i sum_k w_ik logsig(-n_ik) ],   w = softmax_k(T n) or 1 / K
    margin:   L = mean_i sum_k w_ik max(p_i - n_ik, -m) + m,                        w = softmax_k(-T n) or 1 / K
  with the weights constants of the backward pass, the maximum's tie giving half the gradient to each side, and the
  gradient through a modulus that is exactly 0 being 0 (torch's norm backward).

The forward is written in torch and the gradients come from autograd. The same forward evaluated in float32 gives
SCORE_DEV and the cases' own float32 deviation (rotate_cases.py admits a case only if that is small).

GRAD_DEV[family]: the measured worst deviation of the reference implementation's own float32 gradients (the SGD lr 1
table deltas of tests/golden/rotate_g*.npz) from this float64 form, per loss family, rounded up to two digits;
test_rotate_reference_cpu.py measures it again and asserts that it has not grown.
SCORE_DEV[D]: the worst |float32 - float64| / max(1, float64) of this forward evaluated by torch in float32 over the
three modes and both link-prediction sides on score_case(D) (the inputs of the GPU score tests), rounded up to two
digits; pinned to the reference implementation by rotate_p*.npz (its float32 predict is this float32 forward).
Neither table is taken from the kernels.
"""
import numpy as np
import torch

from adv_reference import adam_update, adam_weights, expand_batch, family  # noqa: F401  (re-exported for the tests)

TABLES = ("ent_embeddings", "rel_embeddings")
E, R = 37, 3   # the synthetic cases' table sizes
PI32 = torch.tensor([3.14159265358979323846], dtype=torch.float32)   # BaseModule.pi_const

GRAD_DEV = {
    "sigmoid_adv": 3.0e-8,
    "sigmoid": 6.0e-8,
    "margin_adv": 5.0e-8,
    "margin_model": 2.1e-7,
}

SCORE_DIMS = (5, 8, 20, 200, 260, 512, 1024)
SCORE_DEV = {5: 1.8e-7, 8: 1.5e-7, 20: 1.5e-7, 200: 1.6e-7, 260: 1.6e-7, 512: 1.5e-7, 1024: 1.3e-7}


def phase_div(rel_range):
    """q of phi = r / q from the model's rel_embedding_range (a Python float): double / float32 tensor."""
    return float((float(rel_range) / PI32).item())


def init_ranges(dim, gamma, eps):
    """(ent_embedding_range, rel_embedding_range) as the constructor stores them (float32 parameters)."""
    return (float(torch.Tensor([(gamma + eps) / (2 * dim)]).item()), float(torch.Tensor([(gamma + eps) / dim]).item()))


def _broadcast(table, idx, bs):
    """table[idx] for an index that repeats its first bs entries: gathered once and broadcast, as the models gather the
    fixed side and the relation of a head_batch / tail_batch (autograd then sums over the negatives before it
    scatters)."""
    rows = table[idx[:bs]]
    return rows.unsqueeze(0).expand(idx.numel() // bs, bs, rows.shape[-1]).reshape(idx.numel(), rows.shape[-1])


def slot_vectors(tabs, h, t, r, q, mode="normal", bs=None):
    """(v_re, v_im, |h|, |t|) of every slot ([n, D] tensors) from table tensors (ent [E, 2D], rel [R, D]) of one dtype,
    the batch in the expanded layout. With bs, a head_batch / tail_batch gathers its fixed side and its relation once
    per positive (the same values; the order of the backward pass's sums is the models')."""
    ent, rel = tabs
    D = rel.shape[1]
    compact = bs is not None and mode != "normal"
    hv = _broadcast(ent, h, bs) if compact and mode == "tail_batch" else ent[h]
    tv = _broadcast(ent, t, bs) if compact and mode == "head_batch" else ent[t]
    hr, hi, tr, ti = hv[:, :D], hv[:, D:], tv[:, :D], tv[:, D:]
    phi = (_broadcast(rel, r, bs) if compact else rel[r]) / q
    c, s = torch.cos(phi), torch.sin(phi)
    if mode == "head_batch":
        vr = (c * tr + s * ti) - hr
        vi = (c * ti - s * tr) - hi
    else:
        vr = (hr * c - hi * s) - tr
        vi = (hr * s + hi * c) - ti
    return vr, vi, torch.sqrt(hr * hr + hi * hi), torch.sqrt(tr * tr + ti * ti)


def _modulus(vr, vi):
    return torch.stack([vr, vi], dim=0).norm(dim=0)   # (the reference's form: its backward is 0 at a zero modulus)


def scores(tables, h, t, r, q, mode="normal", dtype=torch.float64):
    """The distances d as a numpy array, evaluated by torch in `dtype` (batch in the expanded layout)."""
    tabs = [torch.tensor(np.asarray(x), dtype=dtype) for x in tables]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    with torch.no_grad():
        vr, vi, _, _ = slot_vectors(tabs, hh, tt, rr, q, mode)
        return _modulus(vr, vi).sum(-1).numpy()


def loss_value(tabs, h, t, r, bs, cfg, mode="normal"):
    """The step's loss (0-dim tensor) and the intermediate tensors, in the tables' dtype."""
    dt = tabs[0].dtype
    vr, vi, ah, at = slot_vectors(tabs, h, t, r, cfg["phase_div"], mode, bs)
    mod = _modulus(vr, vi)
    d = mod.sum(-1)
    s = float(cfg["model_margin"]) - d
    p = s[:bs].view(-1, bs).permute(1, 0)   # [B, 1]
    n = s[bs:].view(-1, bs).permute(1, 0)   # [B, K]
    temp = cfg.get("adv_temperature")
    if cfg["loss"] == "sigmoid":
        ls = torch.nn.functional.logsigmoid
        if temp is not None:
            w = torch.softmax(n * temp, -1).detach()
            loss = -(ls(p).mean() + (w * ls(-n)).sum(-1).mean()) / 2
        else:
            loss = -(ls(p).mean() + ls(-n).mean()) / 2
    else:
        m = torch.tensor(-float(cfg["loss_margin"]), dtype=dt)
        if temp is not None:
            w = torch.softmax(-n * temp, -1).detach()
            loss = (w * torch.max(p - n, m)).sum(-1).mean() - m
        else:
            loss = torch.max(p - n, m).mean() - m
    return loss, dict(d=d, p=p, n=n, mod=mod, ah=ah, at=at)


def loss_and_grads(tables, h, t, r, bs, cfg, mode="normal", dtype=torch.float64):
    """(loss, [gradient of ent, of rel as float64 arrays], aux) of one batch in the expanded layout, evaluated by torch
    in `dtype`; tables = arrays (ent [E, 2D], rel [R, D]). aux: gmax (largest |gradient| element), hinge_gap
    (smallest |p - n + m| of the margin losses, inf otherwise), active (share of (positive, negative) pairs on the
    hinge's sloped branch, nan for sigmoid), d (the distances), min_mod (the smallest modulus of any slot's v), and
    cond = [per table] the first-order conditioning estimate of every gradient cell: the sum over the slots touching
    the cell of |dL/dd_k| * 2^-23 * (|h| + |t|) / |v| at the cell's complex element."""
    tabs = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in tables]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    loss, mid = loss_value(tabs, hh, tt, rr, bs, cfg, mode)
    mid["d"].retain_grad()
    loss.backward()
    grads = [x.grad.double().numpy().copy() if x.grad is not None else np.zeros(tuple(x.shape)) for x in tabs]
    aux = {"gmax": max(float(np.abs(g).max()) for g in grads), "hinge_gap": float("inf"), "active": float("nan"),
           "d": mid["d"].detach().double().numpy().copy(), "min_mod": float(mid["mod"].detach().min())}
    if cfg["loss"] == "margin":
        arg = (mid["p"] - mid["n"] + float(cfg["loss_margin"])).detach()
        aux["hinge_gap"] = float(arg.abs().min())
        aux["active"] = float((arg > 0).double().mean())
    # conditioning estimate
    D = tabs[1].shape[1]
    cd = mid["d"].grad.detach().double().abs().numpy()[:, None]
    mod = mid["mod"].detach().double().numpy()
    ah, at = mid["ah"].detach().double().numpy(), mid["at"].detach().double().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        est = np.where(mod > 0, cd * 2.0 ** -23 * (ah + at) / mod, 0.0)   # [n, D]
    ce, cr = np.zeros(tuple(tabs[0].shape)), np.zeros(tuple(tabs[1].shape))
    hn, tn, rn = (np.asarray(x, dtype=np.int64) for x in (h, t, r))
    for half in (0, D):
        np.add.at(ce[:, half:half + D], hn, est)
        np.add.at(ce[:, half:half + D], tn, est)
    np.add.at(cr, rn, est)
    aux["cond"] = [ce, cr]
    return float(loss.detach()), grads, aux


def grad_bound(fam, gmax):
    """The project's parity bound of a gradient cell (test_gpu_adv.py): four float32 ulps of the largest gradient
    (at least of 1), or four times the reference implementation's own float32 deviation, capped at 1e-5."""
    return min(1e-5, max(4 * 2.0 ** -23 * max(1.0, gmax), 4 * GRAD_DEV[fam]))


def score_tol(D):
    """test_gpu_lp_values.py's rule for a score cell, relative to max(1, score)."""
    return min(1e-5, max(4 * 2.0 ** -23, 4 * SCORE_DEV[D]))


def lp_scores(tables, anchor, r, side, q, dtype=torch.float64):
    """[E] distances of every entity as the missing side of one query: side 0 head prediction (anchor = the tail, the
    head_batch form), side 1 tail prediction (anchor = the head)."""
    n = np.asarray(tables[0]).shape[0]
    cand = np.arange(n, dtype=np.int64)
    fixed = np.full(n, anchor, dtype=np.int64)
    rr = np.full(n, r, dtype=np.int64)
    if side == 0:
        return scores(tables, cand, fixed, rr, q, "head_batch", dtype)
    return scores(tables, fixed, cand, rr, q, "tail_batch", dtype)


# ---------------------------------------------------------------------------------------- fixtures
def golden_cfg(z):
    """The configuration dict of a tests/golden/rotate_g*.npz / rotate_a*.npz file."""
    def opt(key):
        x = float(z[key])
        return None if np.isnan(x) else x
    return {"model": "RotatE", "loss": str(z["loss"]), "adv_temperature": opt("adv_temperature"),
            "loss_margin": opt("loss_margin"), "model_margin": float(z["model_margin"]),
            "epsilon": float(z["epsilon"]), "sampling": str(z["sampling"]), "dim": int(z["dim"]),
            "batch_size": int(z["batch_size"]), "neg_ent": int(z["neg_ent"]), "torch_seed": int(z["torch_seed"]),
            "phase_div": phase_div(float(z["rel_embedding_range"]))}


def golden_tables(z, tag):
    """(ent, rel) arrays stored under `tag` (or untagged) in a golden file."""
    pre = tag + "_" if tag else ""
    return tuple(z[pre + k] for k in TABLES)


def golden_step(z, cfg, s):
    """Step s's batch of a golden run in the expanded layout, and its mode."""
    mode = str(z["modes"][s])
    return expand_batch(z["b%d_h" % s], z["b%d_t" % s], z["b%d_r" % s], mode, cfg["batch_size"]), mode


# ---------------------------------------------------------------------------------------- score cases
SCORE_GAMMA, SCORE_EPS = 6.0, 2.0


def score_case(D):
    """Tables (E = 37, R = 3, at the model's init scale: entities uniform within +-(gamma + eps) / (2 D), phases within
    +-(gamma + eps) / D, i.e. phi within +-pi), the three modes' batches of the score tests at dim D ({mode: (h, t, r)
    as predict takes them}) and the phase divisor."""
    rng = np.random.default_rng(9000 + D)
    er, rr = init_ranges(D, SCORE_GAMMA, SCORE_EPS)
    tabs = [rng.uniform(-er, er, size=(E, 2 * D)).astype(np.float32),
            rng.uniform(-rr, rr, size=(R, D)).astype(np.float32)]
    n = 41
    h, t, r = rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)
    batches = {"normal": (h, t, r), "head_batch": (rng.integers(0, E, n), t[:1], r[:1]),
               "tail_batch": (h[:1], rng.integers(0, E, n), r[:1])}
    return tabs, batches, phase_div(rr)


def expand_predict(h, t, r, mode):
    """predict's head_batch / tail_batch arguments (fixed side and relation of length 1) broadcast."""
    h, t, r = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (h, t, r))
    n = max(h.size, t.size)
    return np.resize(h, n), np.resize(t, n), np.resize(r, n)


def measure_score_dev(D):
    """Worst relative deviation of the float32 torch forward from float64 over score_case(D)."""
    worst = 0.0
    tabs, batches, q = score_case(D)
    for mode, (h, t, r) in batches.items():
        hh, tt, rr = expand_predict(h, t, r, mode)
        ref = scores(tabs, hh, tt, rr, q, mode, torch.float64)
        got = scores(tabs, hh, tt, rr, q, mode, torch.float32).astype(np.float64)
        worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, ref)).max()))
        for side in (0, 1):   # the link-prediction rows of the same tables
            ref = lp_scores(tabs, int(h[0]), int(r[0]), side, q)
            got = lp_scores(tabs, int(h[0]), int(r[0]), side, q, torch.float32).astype(np.float64)
            worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, ref)).max()))
    return worst


def measure_grad_dev(z):
    """Worst |reference float32 gradient - float64 gradient| over the steps of one rotate_g*.npz (the SGD lr 1 table
    deltas against this form at the tables before each step)."""
    cfg = golden_cfg(z)
    worst = 0.0
    for s in range(int(z["steps"])):
        (h, t, r), mode = golden_step(z, cfg, s)
        before, after = golden_tables(z, "s%d" % s), golden_tables(z, "s%d" % (s + 1))
        _, grads, _ = loss_and_grads(before, h, t, r, cfg["batch_size"], cfg, mode)
        for b, a, g in zip(before, after, grads):
            worst = max(worst, float(np.abs((b.astype(np.float64) - a.astype(np.float64)) - g).max()))
    return worst
