"""The synthetic cases of tests/test_gpu_adv.py, shared with tests/test_adv_reference_cpu.py (which checks their
input conditions on the CPU): tables uniform(-1, 1) * scale from a seeded generator over E = 6 entities and R = 2
relations, so every step holds repeated corrupted entities (within a positive and across positives) and negatives
equal to the positive's own rows; batches given explicitly."""
import numpy as np

E, R = 6, 2

# id, D, B, K, mode, norm_flag, p, loss, adv_temperature, loss margin, model margin, table scale, seed
GRAD_CASES = [
    ("d5-k1", 5, 1, 1, "normal", True, 1, "sigmoid", 1.0, None, 6.0, 1.0, 1),
    ("d20-p2", 20, 5, 3, "normal", False, 2, "sigmoid", 0.5, None, None, 1.0, 2),
    ("d23-b33-head", 23, 33, 3, "head_batch", True, 1, "sigmoid", None, None, 4.0, 1.0, 3),
    ("d69-k64-tail", 69, 5, 64, "tail_batch", False, 1, "sigmoid", 1.0, None, 6.0, 0.1, 4),
    ("d200-k65-head", 200, 5, 65, "head_batch", True, 2, "margin", 1.0, 3.0, None, 1.0, 5),
    ("d500-k130", 500, 5, 130, "normal", False, 2, "margin", 2.0, 5.0, 6.0, 0.1, 6),
    ("d512-b33-tail", 512, 33, 3, "tail_batch", True, 2, "margin", None, 4.0, 5.0, 1.0, 7),
    ("d512-p1", 512, 5, 3, "normal", False, 1, "sigmoid", 1.0, None, 6.0, 0.02, 8),
    ("d20-k130-head", 20, 5, 130, "head_batch", True, 1, "margin", None, 2.0, 3.0, 1.0, 9),
    ("d23-k65", 23, 1, 65, "normal", True, 2, "sigmoid", None, None, None, 1.0, 10),
    ("d8-k130-tail", 8, 33, 130, "tail_batch", True, 2, "sigmoid", 1.0, None, 6.0, 1.0, 11),
    ("d20-k256-head", 20, 1, 256, "head_batch", False, 2, "margin", 1.0, 3.0, None, 1.0, 12),
]
# distances around 30, temperature 40, unnormalised rows scaled by 8
STABILITY_CASE = ("stability", 5, 5, 64, "normal", False, 1, "sigmoid", 40.0, None, 6.0, 8.0, 13)
ADAGRAD_CASE = ("adagrad", 20, 5, 3, "normal", True, 1, "sigmoid", 1.0, None, 6.0, 1.0, 14)
ALL_CASES = GRAD_CASES + [STABILITY_CASE, ADAGRAD_CASE]


def case_cfg(case):
    _, D, B, K, mode, nf, p, loss, temp, lmargin, gamma, scale, seed = case
    return {"model": "TransE", "loss": loss, "adv_temperature": temp, "loss_margin": lmargin, "p_norm": p,
            "norm_flag": nf, "model_margin": gamma, "dim": D, "batch_size": B, "neg_ent": K}


def make_tables(rng, D, scale, ent=E, rel=R, transh=False):
    out = [(rng.uniform(-1, 1, size=(ent, D)) * scale).astype(np.float32),
           (rng.uniform(-1, 1, size=(rel, D)) * scale).astype(np.float32)]
    out.append((rng.uniform(-1, 1, size=(rel, D)) * scale).astype(np.float32) if transh else None)
    return out


def make_batch(rng, B, K, mode, ent=E, rel=R):
    """A batch dict as Trainer.train_one_step takes it: normal mode corrupts the tail, the head or (about one slot
    in ten) the relation of each negative; head_batch / tail_batch give the fixed side and the relation once."""
    h = rng.integers(0, ent, size=B)
    t = rng.integers(0, ent, size=B)
    r = rng.integers(0, rel, size=B)
    n = B * K
    if mode == "normal":
        hh, tt, rr = np.tile(h, K), np.tile(t, K), np.tile(r, K)
        what = rng.random(n)
        new_e = rng.integers(0, ent, size=n)
        new_r = rng.integers(0, rel, size=n)
        tt = np.where(what < 0.45, new_e, tt)
        hh = np.where((what >= 0.45) & (what < 0.9), new_e, hh)
        rr = np.where(what >= 0.9, new_r, rr)
        bh, bt, br = np.concatenate([h, hh]), np.concatenate([t, tt]), np.concatenate([r, rr])
    elif mode == "head_batch":
        bh, bt, br = np.concatenate([h, rng.integers(0, ent, size=n)]), t, r
    else:
        bh, bt, br = h, np.concatenate([t, rng.integers(0, ent, size=n)]), r
    return {"batch_h": bh.astype(np.int64), "batch_t": bt.astype(np.int64), "batch_r": br.astype(np.int64),
            "batch_y": np.zeros(B * (K + 1), dtype=np.float32), "mode": mode}


# Adam: three steps from a given state over 8 entities; entity 6 appears in step 1 only (as a corrupted tail),
# entity 7 never; entity rows 0-5 and the relation tables start with nonzero moments, entity rows 6 and 7 with zero
# id, model, D, B, K, norm_flag, p, loss, adv_temperature, loss margin, model margin, lr, first step, seed
ADAM_CASES = [
    ("adam-transe", "TransE", 20, 5, 3, True, 1, "sigmoid", 1.0, None, 6.0, 1e-3, 5, 21),
    ("adam-transh", "TransH", 12, 5, 2, True, 2, "margin", None, 3.0, None, 1e-3, 0, 22),
]
ADAM_ENT, ADAM_STEPS = 8, 3


def build_adam(case):
    """(tables, [batch per step], cfg, (m0, v0) per table, lr, steps already done)."""
    _, model, D, B, K, nf, p, loss, temp, lmargin, gamma, lr, step0, seed = case
    rng = np.random.default_rng(2000 + seed)
    transh = model == "TransH"
    tabs = make_tables(rng, D, 1.0, ent=ADAM_ENT, transh=transh)
    batches = [make_batch(rng, B, K, "normal", ent=6) for _ in range(ADAM_STEPS)]
    batches[0]["batch_t"][B] = 6       # negative 0 of positive 0 and of positive 2: corrupted tail = entity 6
    batches[0]["batch_h"][B] = batches[0]["batch_h"][0]
    batches[0]["batch_r"][B] = batches[0]["batch_r"][0]
    batches[0]["batch_t"][B + 2] = 6
    batches[0]["batch_h"][B + 2] = batches[0]["batch_h"][2]
    batches[0]["batch_r"][B + 2] = batches[0]["batch_r"][2]
    m0, v0 = [], []
    for x in tabs:
        if x is None:
            m0.append(None); v0.append(None)
            continue
        m = (0.01 * rng.uniform(-1, 1, size=x.shape)).astype(np.float32)
        v = (1e-5 * rng.uniform(0, 1, size=x.shape)).astype(np.float32)
        if x.shape[0] == ADAM_ENT:
            m[6:] = 0
            v[6:] = 0
        m0.append(m); v0.append(v)
    cfg = {"model": model, "loss": loss, "adv_temperature": temp, "loss_margin": lmargin, "p_norm": p,
           "norm_flag": nf, "model_margin": gamma, "dim": D, "batch_size": B, "neg_ent": K}
    return tabs, batches, cfg, (m0, v0), lr, step0


def build(case):
    """(tables, batch dict, cfg) of a case."""
    _, D, B, K, mode, nf, p, loss, temp, lmargin, gamma, scale, seed = case
    rng = np.random.default_rng(1000 + seed)
    return make_tables(rng, D, scale), make_batch(rng, B, K, mode), case_cfg(case)
