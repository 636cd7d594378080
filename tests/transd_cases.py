"""The synthetic cases of tests/test_gpu_transd.py, shared with tests/test_transd_reference_cpu.py (which checks their
input conditions on the CPU): four tables uniform(-1, 1) * scale from a seeded generator over E = 37 entities and
R = 3 relations, so rows collide constantly; batches given explicitly. Entity 36 and relation 2 are never drawn (their
rows must stay bit-identical); every batch carries planted slots (plant()).

The loss margins are chosen so that between 20 % and 80 % of the (positive, negative) pairs are active: with a margin
of the size of the distances every pair would be, and the inactive branch untested."""
import numpy as np

from transd_reference import E, R

FREE_ENT, FREE_REL = E - 1, R - 1   # never in a batch

# id, D, B, K, mode, norm_flag, p, loss margin, table scale, seed
GRAD_CASES = [
    ("d5-p1", 5, 11, 3, "normal", True, 1, 0.05, 1.0, 1),           # VEC 1
    ("d5-p2-raw-head", 5, 11, 7, "head_batch", False, 2, 0.05, 1.0, 2),
    ("d8-p2", 8, 37, 3, "normal", True, 2, 0.05, 1.0, 3),           # float4, G = 2
    ("d8-p1-raw-tail", 8, 11, 1, "tail_batch", False, 1, 0.1, 1.0, 4),
    ("d20-p1-raw", 20, 37, 7, "normal", False, 1, 0.2, 1.0, 5),     # the experiment's dim
    ("d20-p2-head", 20, 11, 3, "head_batch", True, 2, 0.02, 1.0, 6),
    ("d200-p1", 200, 11, 3, "normal", True, 1, 0.2, 1.0, 7),        # G = 64 with 14 idle lanes; the example's dim
    ("d200-p2-raw-tail", 200, 37, 1, "tail_batch", False, 2, 0.01, 1.0, 8),
    ("d260-p2-raw", 260, 11, 7, "normal", False, 2, 0.01, 1.0, 9),  # KCH = 2 with a partial second chunk
    ("d260-p1-head", 260, 11, 1, "head_batch", True, 1, 0.2, 1.0, 10),
    ("d512-p2", 512, 37, 3, "normal", True, 2, 0.01, 1.0, 11),      # the widest
    ("d512-p1-raw-tail", 512, 11, 1, "tail_batch", False, 1, 0.3, 1.0, 20),
]
ADAGRAD_CASE = ("adagrad", 20, 11, 3, "normal", True, 1, 0.1, 1.0, 13)
ALL_CASES = GRAD_CASES + [ADAGRAD_CASE]


def case_cfg(case):
    _, D, B, K, mode, nf, p, margin, scale, seed = case
    return {"model": "TransD", "p_norm": p, "norm_flag": nf, "dim": D, "batch_size": B, "neg_ent": K,
            "loss_margin": margin}


def make_tables(rng, D, scale, ent=E, rel=R):
    return [(rng.uniform(-1, 1, size=(rows, D)) * scale).astype(np.float32) for rows in (ent, rel, ent, rel)]


def make_batch(rng, B, K, mode, ent=FREE_ENT, rel=FREE_REL):
    """The expanded-layout batch (h, t, r of length B * (K + 1)) of a mode: every negative keeps its positive's
    relation and replaces the tail or the head (normal: either; head_batch: the head; tail_batch: the tail); then the
    planted slots."""
    h = rng.integers(0, ent, size=B)
    t = rng.integers(0, ent, size=B)
    r = rng.integers(0, rel, size=B)
    n = B * K
    hh, tt, rr = np.tile(h, K), np.tile(t, K), np.tile(r, K)
    new_e = rng.integers(0, ent, size=n)
    if mode == "normal":
        tails = rng.random(n) < 0.5
    else:
        tails = np.full(n, mode == "tail_batch")
    tt = np.where(tails, new_e, tt)
    hh = np.where(~tails, new_e, hh)
    bh, bt, br = np.concatenate([h, hh]), np.concatenate([t, tt]), np.concatenate([r, rr])
    return plant(bh.astype(np.int64), bt.astype(np.int64), br.astype(np.int64), B, K, mode)


def plant(bh, bt, br, B, K, mode):
    """Planted slots (B >= 11): positive 0 a self-loop; negative 0 of positive 1 equal to its positive; in normal
    mode negative 0 of positive 2 with the other relation (the six-row path); positive 3's head = the corrupted
    entity of negative 0 of positive 4 (as a tail in normal / tail_batch mode, as a head in head_batch mode)."""
    bt[0] = bh[0]
    for k in range(K):   # positive 0's negatives keep the side their mode fixes
        o = (k + 1) * B
        if mode == "head_batch" or (mode == "normal" and bh[o] != bh[0] and bt[o] != bt[0]):
            bt[o] = bt[0]
        elif mode == "tail_batch":
            bh[o] = bh[0]
    o = B + 1
    bh[o], bt[o], br[o] = bh[1], bt[1], br[1]
    if mode == "normal":
        o = B + 2
        bh[o], bt[o], br[o] = bh[2], bt[2], 1 - br[2]
    o = B + 4
    if mode == "head_batch":
        bh[o], bt[o], br[o] = bh[3], bt[4], br[4]
    else:
        bh[o], bt[o], br[o] = bh[4], bh[3], br[4]
    return bh, bt, br


def planted(bh, bt, br, B, K, mode):
    """Which planted slot kinds a batch holds."""
    hn, tn, rn = (x[B:].reshape(K, B) for x in (bh, bt, br))
    hp, tp, rp = bh[:B], bt[:B], br[:B]
    out = {"self_loop": bool((hp == tp).any()),
           "neg_equals_pos": bool(((hn == hp) & (tn == tp) & (rn == rp)).any()),
           "other_relation": bool((rn != rp).any()),
           "free_entity": FREE_ENT not in bh and FREE_ENT not in bt, "free_relation": FREE_REL not in br}
    corrupted = np.where(hn != hp, hn, np.where(tn != tp, tn, -1))
    side_tail = (tn != tp) & (hn == hp)
    shared = False
    for i in range(B):
        other = np.ones(B, dtype=bool)
        other[i] = False
        sel = (corrupted[:, other] == hp[i])
        if mode != "head_batch":
            sel &= side_tail[:, other]
        shared |= bool(sel.any())
    out["head_is_other_corrupted"] = shared
    return out


def build(case):
    """(tables, (h, t, r) expanded, cfg, mode) of a case."""
    _, D, B, K, mode, nf, p, margin, scale, seed = case
    rng = np.random.default_rng(3000 + seed)
    return make_tables(rng, D, scale), make_batch(rng, B, K, mode), case_cfg(case), mode


def as_batch(hrt, B, mode):
    """The batch dict Trainer.train_one_step takes: head_batch / tail_batch give the fixed side and the relation once
    per positive."""
    h, t, r = hrt
    if mode == "head_batch":
        t, r = t[:B], r[:B]
    elif mode == "tail_batch":
        h, r = h[:B], r[:B]
    return {"batch_h": h, "batch_t": t, "batch_r": r, "batch_y": np.zeros(len(hrt[0]), dtype=np.float32),
            "mode": mode}


# Adam: three steps from a given state; entity 35 appears in step 1 only (as a corrupted tail), entity 36 never; entity
# rows 0-34 and the relation tables start with nonzero moments, entity rows 35 and 36 with zero
# id, D, B, K, norm_flag, p, loss margin, lr, first step, seed
ADAM_CASES = [
    ("adam-p1", 20, 11, 3, True, 1, 0.1, 1e-3, 5, 21),
    ("adam-p2-raw", 12, 11, 2, False, 2, 0.02, 1e-3, 0, 22),
]
ADAM_STEPS = 3
ONCE_ENT = E - 2


def build_adam(case):
    """(tables, [expanded batch per step], cfg, (m0, v0) per table, lr, steps already done)."""
    _, D, B, K, nf, p, margin, lr, step0, seed = case
    rng = np.random.default_rng(4000 + seed)
    tabs = make_tables(rng, D, 1.0)
    batches = [make_batch(rng, B, K, "normal", ent=ONCE_ENT) for _ in range(ADAM_STEPS)]
    bh, bt, br = batches[0]
    for i in (5, 6):   # negative 0 of positives 5 and 6: corrupted tail = entity 35
        o = B + i
        bh[o], bt[o], br[o] = bh[i], ONCE_ENT, br[i]
    m0, v0 = [], []
    for x in tabs:
        m = (0.01 * rng.uniform(-1, 1, size=x.shape)).astype(np.float32)
        v = (1e-5 * rng.uniform(0, 1, size=x.shape)).astype(np.float32)
        if x.shape[0] == E:
            m[ONCE_ENT:] = 0
            v[ONCE_ENT:] = 0
        m0.append(m); v0.append(v)
    cfg = {"model": "TransD", "p_norm": p, "norm_flag": nf, "dim": D, "batch_size": B, "neg_ent": K,
           "loss_margin": margin}
    return tabs, batches, cfg, (m0, v0), lr, step0
