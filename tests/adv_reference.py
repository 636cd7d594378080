"""Float64 reference of the weighted training step and of dense Adam, written for these tests.

  d = ||h^ + r^ - t^||_p (rows L2-normalised under norm_flag, eps 1e-12; TransH projects h and t onto the relation's
  hyperplane first); score s = gamma - d when the model carries a margin, else d. A batch holds B positives with K
  negatives each, negative k of positive i at (k + 1) * B + i.
    sigmoid:  L = -1/2 [ mean_i logsig(p_i) + mean_i sum_k w_ik logsig(-n_ik) ],   w = softmax_k(T n) or 1 / K
    margin:   L = mean_i sum_k w_ik max(p_i - n_ik, -m) + m,                        w = softmax_k(-T n) or 1 / K
  with the weights constants of the backward pass and the maximum's tie giving half the gradient to each side.

The forward is written in torch float64 and the gradients come from autograd, so every table (norm_vector included)
has a reference. Adam is torch.optim.Adam's update (no weight decay, no amsgrad) written out.

GRAD_DEV: the measured worst deviation of the reference implementation's own float32 gradients (the SGD lr 1 table
deltas of tests/golden/adv_g*.npz) from this float64 form, per case family, rounded up to two digits;
test_adv_reference_cpu.py measures it again and asserts that it has not grown.
"""
import numpy as np
import torch

EPS_NORMALIZE = 1e-12

# family -> worst |float32 reference gradient - float64 gradient| over the family's golden cases
GRAD_DEV = {
    "sigmoid_adv": 3.0e-8,
    "sigmoid": 3.4e-8,
    "margin_adv": 1.1e-7,
    "margin_model": 3.7e-8,
}


def family(cfg):
    if cfg["loss"] == "sigmoid":
        return "sigmoid_adv" if cfg.get("adv_temperature") is not None else "sigmoid"
    return "margin_adv" if cfg.get("adv_temperature") is not None else "margin_model"


def expand_batch(h, t, r, mode, bs):
    """The batch in the expanded normal-mode layout: head_batch / tail_batch give the uncorrupted side and the
    relation once per positive (the first bs entries are used, as the models' views do)."""
    h, t, r = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (h, t, r))
    if mode == "normal":
        return h, t, r
    full = h if mode == "head_batch" else t
    rep = full.size // bs
    if mode == "head_batch":
        t = np.tile(t[:bs], rep)
    else:
        h = np.tile(h[:bs], rep)
    return h, t, np.tile(r[:bs], rep)


def _normalize(x):
    return x / x.norm(2, -1, keepdim=True).clamp_min(EPS_NORMALIZE)


def slot_vectors(tabs, h, t, r, cfg):
    """v = h^ + r^ - t^ of every slot ([n, D] float64 tensor) from float64 table tensors (ent, rel[, norm])."""
    ent, rel = tabs[0], tabs[1]
    hv, tv, rv = ent[h], ent[t], rel[r]
    if cfg.get("model", "TransE") == "TransH":
        nv = _normalize(tabs[2][r])
        hv = hv - (hv * nv).sum(-1, keepdim=True) * nv
        tv = tv - (tv * nv).sum(-1, keepdim=True) * nv
    if cfg["norm_flag"]:
        hv, rv, tv = _normalize(hv), _normalize(rv), _normalize(tv)
    return (hv + rv) - tv


def loss_value(tabs, h, t, r, bs, cfg):
    """The step's loss (0-dim float64 tensor) and the intermediate tensors (v, d, p, n)."""
    v = slot_vectors(tabs, h, t, r, cfg)
    d = v.norm(cfg["p_norm"], -1)
    gamma = cfg.get("model_margin")
    s = gamma - d if gamma is not None else d
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
        m = torch.tensor(-float(cfg["loss_margin"]), dtype=torch.float64)
        if temp is not None:
            w = torch.softmax(-n * temp, -1).detach()
            loss = (w * torch.max(p - n, m)).sum(-1).mean() - m
        else:
            loss = torch.max(p - n, m).mean() - m
    return loss, dict(v=v, d=d, p=p, n=n)


def loss_and_grads(tables, h, t, r, bs, cfg):
    """(loss, [gradient per table as float64 arrays], aux) of one batch in the expanded layout; tables = float32 or
    float64 arrays (ent, rel[, norm_vector]). aux: min_abs_v (smallest |component| of any slot's v), hinge_gap
    (smallest |p - n + m| of the margin losses, inf otherwise), gmax (largest |gradient| element)."""
    tabs = [torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True) for x in tables if x is not None]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    loss, mid = loss_value(tabs, hh, tt, rr, bs, cfg)
    loss.backward()
    grads = [x.grad.numpy().copy() if x.grad is not None else np.zeros(tuple(x.shape)) for x in tabs]
    aux = {"min_abs_v": float(mid["v"].detach().abs().min()), "hinge_gap": float("inf"),
           "gmax": max(float(np.abs(g).max()) for g in grads), "d": mid["d"].detach().numpy().copy()}
    if cfg["loss"] == "margin":
        aux["hinge_gap"] = float((mid["p"] - mid["n"] + float(cfg["loss_margin"])).detach().abs().min())
    return float(loss.detach()), grads, aux


def adam_update(w, m, v, g, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """One dense Adam step in float64 (step counts from 1): returns (w', m', v')."""
    w, m, v, g = (np.asarray(x, dtype=np.float64) for x in (w, m, v, g))
    m2 = m + (1.0 - beta1) * (g - m)
    v2 = beta2 * v + (1.0 - beta2) * g * g
    return adam_weights(w, m2, v2, lr, step, beta1, beta2, eps), m2, v2


def adam_weights(w, m_new, v_new, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """w' of a dense Adam step from the pre-step weights and the post-step moments, in float64."""
    w, m_new, v_new = (np.asarray(x, dtype=np.float64) for x in (w, m_new, v_new))
    step_size = lr / (1.0 - beta1 ** step)
    denom = np.sqrt(v_new) / np.sqrt(1.0 - beta2 ** step) + eps
    return w - step_size * m_new / denom


def golden_cfg(z):
    """The configuration dict of a tests/golden/adv_*.npz file."""
    def opt(key):
        x = float(z[key])
        return None if np.isnan(x) else x
    return {"model": str(z["model"]), "loss": str(z["loss"]), "adv_temperature": opt("adv_temperature"),
            "loss_margin": opt("loss_margin"), "p_norm": int(z["p_norm"]), "norm_flag": bool(z["norm_flag"]),
            "model_margin": opt("model_margin"), "epsilon": opt("epsilon"), "sampling": str(z["sampling"]),
            "dim": int(z["dim"]), "batch_size": int(z["batch_size"]), "neg_ent": int(z["neg_ent"])}


def golden_tables(z, tag):
    """(ent, rel, norm_vector or None) arrays stored under `tag` in a golden file."""
    nv = tag + "_norm_vector"
    return (z[tag + "_ent_embeddings"], z[tag + "_rel_embeddings"], z[nv] if nv in z.files else None)
