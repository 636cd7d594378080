"""Float64 reference of TransD (dim_e == dim_r) written for these tests: forward, MarginLoss step, link-prediction
scores.

  N(x) = x / max(||x||_2, 1e-12);  u_e = e + (e . e_p) r_p;  e_perp = N(u_e) (always);
  under norm_flag e_perp <- N(e_perp) and r <- N(r);  d = ||(h_perp + r) - t_perp||_p  (head_batch: h_perp + (r - t_perp)).
  A batch holds B positives with K negatives each, negative k of positive i at (k + 1) * B + i;
  L = mean_{i,k} max(p_i - n_ik, -m) + m, the maximum's tie giving half the gradient to each side.

The forward is written in torch and the gradients come from autograd, for all four tables (ent, rel, ent_transfer,
rel_transfer). The same forward evaluated in float32 gives SCORE_DEV.

GRAD_DEV[family]: the measured worst deviation of the reference implementation's own float32 gradients (the SGD lr 1
table deltas of tests/golden/transd_g*.npz) from this float64 form, per (p, norm_flag) family, rounded up to two
digits; test_transd_reference_cpu.py measures it again and asserts that it has not grown.
SCORE_DEV[D]: the worst |float32 - float64| / max(1, float64) of this forward evaluated by torch in float32, over
p x norm_flag x the three modes on score_case(D, p, norm_flag) (the inputs of the GPU score tests), rounded up to two
digits; pinned to the reference implementation by transd_p*.npz (its float32 predict is this float32 forward).
Neither table is taken from the kernels.
"""
import numpy as np
import torch

from adv_reference import adam_update, adam_weights, expand_batch  # noqa: F401  (re-exported for the tests)

EPS_NORMALIZE = 1e-12
TABLES = ("ent_embeddings", "rel_embeddings", "ent_transfer", "rel_transfer")
E, R = 37, 3   # the synthetic cases' table sizes

GRAD_DEV = {
    "p1_norm": 6.5e-8,
    "p1_raw": 5.2e-8,
    "p2_norm": 3.0e-8,
    "p2_raw": 2.8e-8,
}

SCORE_DIMS = (5, 8, 20, 200, 260, 512)
SCORE_DEV = {5: 1.6e-7, 8: 1.9e-7, 20: 2.4e-7, 200: 5.4e-7, 260: 6.3e-7, 512: 1.3e-6}


def family(cfg):
    return "p%d_%s" % (cfg["p_norm"], "norm" if cfg["norm_flag"] else "raw")


def _normalize(x):
    return x / x.norm(2, -1, keepdim=True).clamp_min(EPS_NORMALIZE)


def _project(ent, ent_t, rel_t, e, r):
    ev = ent[e]
    u = ev + (ev * ent_t[e]).sum(-1, keepdim=True) * rel_t[r]
    return _normalize(u), u


def distances(tabs, h, t, r, cfg, mode="normal"):
    """d of every slot (tensor [n]) from table tensors (ent, rel, ent_transfer, rel_transfer) of one dtype, the batch
    in the expanded layout; also the two u tensors."""
    ent, rel, ent_t, rel_t = tabs
    hv, uh = _project(ent, ent_t, rel_t, h, r)
    tv, ut = _project(ent, ent_t, rel_t, t, r)
    rv = rel[r]
    if cfg["norm_flag"]:
        hv, rv, tv = _normalize(hv), _normalize(rv), _normalize(tv)
    v = hv + (rv - tv) if mode == "head_batch" else (hv + rv) - tv
    return v.norm(cfg["p_norm"], -1), v, uh, ut


def scores(tables, h, t, r, cfg, mode="normal", dtype=torch.float64):
    """model.predict's distances as a numpy array, evaluated by torch in `dtype` (batch in the expanded layout)."""
    tabs = [torch.tensor(np.asarray(x), dtype=dtype) for x in tables]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    with torch.no_grad():
        return distances(tabs, hh, tt, rr, cfg, mode)[0].numpy()


def loss_and_grads(tables, h, t, r, bs, cfg, mode="normal"):
    """(loss, [gradient per table as float64 arrays], aux) of one batch in the expanded layout; tables = float32 or
    float64 arrays (ent, rel, ent_transfer, rel_transfer). aux: min_abs_v (smallest |component| of any slot's v),
    hinge_gap (smallest |p - n + m|), gmax (largest |gradient| element), min_u (smallest ||u|| of any projected
    side), active (share of (positive, negative) pairs with p - n > -m), d (the distances)."""
    tabs = [torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True) for x in tables]
    hh, tt, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    d, v, uh, ut = distances(tabs, hh, tt, rr, cfg, mode)
    p = d[:bs].view(-1, bs).permute(1, 0)
    n = d[bs:].view(-1, bs).permute(1, 0)
    m = float(cfg["loss_margin"])
    loss = torch.max(p - n, torch.tensor(-m, dtype=torch.float64)).mean() + m
    loss.backward()
    grads = [x.grad.numpy().copy() if x.grad is not None else np.zeros(tuple(x.shape)) for x in tabs]
    arg = (p - n + m).detach()
    aux = {"min_abs_v": float(v.detach().abs().min()), "hinge_gap": float(arg.abs().min()),
           "gmax": max(float(np.abs(g).max()) for g in grads),
           "min_u": float(min(uh.detach().norm(2, -1).min(), ut.detach().norm(2, -1).min())),
           "active": float((arg > 0).double().mean()), "d": d.detach().numpy().copy()}
    return float(loss.detach()), grads, aux


def grad_bound(fam, gmax):
    """The project's parity bound of a gradient cell (test_gpu_adv.py): four float32 ulps of the largest gradient
    (at least of 1), or four times the reference implementation's own float32 deviation, capped at 1e-5."""
    return min(1e-5, max(4 * 2.0 ** -23 * max(1.0, gmax), 4 * GRAD_DEV[fam]))


def score_tol(D):
    """test_gpu_lp_values.py's rule for a score cell, relative to max(1, score)."""
    return min(1e-5, max(4 * 2.0 ** -23, 4 * SCORE_DEV[D]))


def lp_scores(tables, anchor, r, side, cfg, dtype=torch.float64):
    """[E] scores of every entity as the missing side of one query: side 0 head prediction (anchor = the tail,
    association e + (r - t)), side 1 tail prediction (anchor = the head, (h + r) - e)."""
    n = np.asarray(tables[0]).shape[0]
    cand = np.arange(n, dtype=np.int64)
    fixed = np.full(n, anchor, dtype=np.int64)
    rr = np.full(n, r, dtype=np.int64)
    if side == 0:
        return scores(tables, cand, fixed, rr, cfg, "head_batch", dtype)
    return scores(tables, fixed, cand, rr, cfg, "tail_batch", dtype)


# ---------------------------------------------------------------------------------------- fixtures
def golden_cfg(z):
    """The configuration dict of a tests/golden/transd_g*.npz / transd_a*.npz file."""
    return {"model": "TransD", "p_norm": int(z["p_norm"]), "norm_flag": bool(z["norm_flag"]),
            "sampling": str(z["sampling"]), "dim": int(z["dim"]), "batch_size": int(z["batch_size"]),
            "neg_ent": int(z["neg_ent"]), "loss_margin": float(z["loss_margin"]),
            "model_margin": None if np.isnan(float(z["model_margin"])) else float(z["model_margin"]),
            "epsilon": None if np.isnan(float(z["epsilon"])) else float(z["epsilon"]),
            "torch_seed": int(z["torch_seed"])}


def golden_tables(z, tag):
    """(ent, rel, ent_transfer, rel_transfer) arrays stored under `tag` (or untagged) in a golden file."""
    pre = tag + "_" if tag else ""
    return tuple(z[pre + k] for k in TABLES)


def golden_step(z, cfg, s):
    """Step s's batch of a golden run in the expanded layout, and its mode."""
    mode = str(z["modes"][s])
    return expand_batch(z["b%d_h" % s], z["b%d_t" % s], z["b%d_r" % s], mode, cfg["batch_size"]), mode


# ---------------------------------------------------------------------------------------- score cases
def score_case(D, p, nf):
    """Tables (E = 37, R = 3, uniform(-1, 1)) and the three modes' batches of the score tests at dim D:
    {mode: (h, t, r) as predict takes them}."""
    rng = np.random.default_rng(7000 + 10 * D + 2 * p + int(nf))
    tabs = [rng.uniform(-1, 1, size=(rows, D)).astype(np.float32) for rows in (E, R, E, R)]
    n = 41
    h, t, r = rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)
    batches = {"normal": (h, t, r), "head_batch": (rng.integers(0, E, n), t[:1], r[:1]),
               "tail_batch": (h[:1], rng.integers(0, E, n), r[:1])}
    return tabs, batches, {"p_norm": p, "norm_flag": nf, "dim": D}


def expand_predict(h, t, r, mode):
    """predict's head_batch / tail_batch arguments (fixed side and relation of length 1) broadcast."""
    h, t, r = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (h, t, r))
    n = max(h.size, t.size)
    return np.resize(h, n), np.resize(t, n), np.resize(r, n)


def measure_score_dev(D):
    """Worst relative deviation of the float32 torch forward from float64 over score_case(D, ...)."""
    worst = 0.0
    for p in (1, 2):
        for nf in (True, False):
            tabs, batches, cfg = score_case(D, p, nf)
            for mode, (h, t, r) in batches.items():
                hh, tt, rr = expand_predict(h, t, r, mode)
                ref = scores(tabs, hh, tt, rr, cfg, mode, torch.float64)
                got = scores(tabs, hh, tt, rr, cfg, mode, torch.float32).astype(np.float64)
                worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, ref)).max()))
                for side in (0, 1):   # the link-prediction rows of the same tables
                    ref = lp_scores(tabs, int(h[0]), int(r[0]), side, cfg)
                    got = lp_scores(tabs, int(h[0]), int(r[0]), side, cfg, torch.float32).astype(np.float64)
                    worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, ref)).max()))
    return worst
