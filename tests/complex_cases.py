"""The synthetic cases of tests/test_gpu_complex.py, shared with tests/test_complex_reference_cpu.py (which checks
their input conditions on the CPU): E = 37 entities and R = 3 relations, so rows collide constantly; normal-mode batches
given explicitly (transd_cases.make_batch: entity 36 and relation 2 are never drawn, and every batch carries the planted
slots of transd_cases.plant: a positive self-loop, a negative equal to its positive, a negative with another relation, a
positive's head equal to another positive's corrupted entity).

Tables are uniform(+-a) with a = sqrt(3) (0.75 / sqrt(dim))^(1/3) (complex_reference.table_scale): the scores then have
a standard deviation near 1.5, both sigmoid branches alive, |g|max below 1.

A case is admitted (admission(), asserted in test_complex_reference_cpu.py) only if
  1. torch's own float32 gradients of the case are within a quarter of the cell bound of the float64 ones;
  2. the scores span at least [-2, 2];
  3. with regul_rate, some gradient cell moves by more than 20 times its bound when the regulariser is switched off in
     the reference;
  4. flipping the sign of the h_im t_re r_im term in the reference, and separately zeroing both im tables, each move
     some gradient cell of every one of the four tables by more than 20 bounds: a kernel with the sign wrong, or one
     that ignores the im half, cannot pass.
No cell is exempted in the GPU tests. Seeds searched: one per case - every case's first seed (its last column, added to
7000, or to 8000 for the Adam cases) met all four conditions (worst figures: float32 deviation 0.19 of the bound,
d20-k70-sig-adv-reg; regulariser effect 191 bounds, d1024-sig-adv-reg; wrong-model effect 16,578 bounds,
d1024-k130-sig-adv)."""
import numpy as np
import torch

import complex_reference as cr
from complex_reference import E, R
from transd_cases import FREE_ENT, FREE_REL, make_batch, plant, planted  # noqa: F401  (re-exported)

# id, D, B, K, loss, adv temperature, regul_rate, seed
GRAD_CASES = [
    ("d1-sig-adv", 1, 11, 3, "sigmoid", 0.5, 0.0, 1),                 # VEC 1, G = 2, one idle lane
    ("d2-soft-reg", 2, 11, 7, "softplus", None, 1.0, 2),
    ("d3-sig", 3, 37, 1, "sigmoid", None, 0.0, 3),
    ("d5-soft-adv-reg", 5, 37, 3, "softplus", 1.0, 1.0, 4),
    ("d8-sig-adv", 8, 37, 7, "sigmoid", 0.5, 0.0, 5),                 # float4, G = 2
    ("d20-soft-reg", 20, 37, 3, "softplus", None, 1.0, 6),
    ("d200-soft-reg", 200, 37, 7, "softplus", None, 1.0, 7),          # the example's dim; idle lanes in the last chunk
    ("d260-sig", 260, 37, 3, "sigmoid", None, 0.0, 8),                # 2 pieces, the second 1 chunk
    ("d512-sig-adv-reg", 512, 37, 7, "sigmoid", 0.5, 1.0, 9),         # 2 whole pieces
    ("d516-soft", 516, 37, 3, "softplus", None, 0.0, 10),             # 3 pieces
    ("d1024-sig-adv-reg", 1024, 37, 7, "sigmoid", 0.5, 1.0, 11),      # 4 pieces
    ("d8-k70-sig-adv", 8, 11, 70, "sigmoid", 0.5, 0.0, 12),           # K > G: strided softmax loops
    ("d20-k70-sig-adv-reg", 20, 11, 70, "sigmoid", 1.0, 1.0, 14),
    ("d1024-k130-sig-adv", 1024, 37, 130, "sigmoid", 0.5, 0.0, 13),
]
# an entity's two rows scaled so that some score exceeds 20: nn.Softplus's threshold branch
THRESHOLD_CASE = ("d20-soft-threshold", 20, 11, 3, "softplus", None, 0.0, 101)
THRESHOLD_SCALE = 12.0
ADAGRAD_CASE = ("adagrad-reg", 20, 37, 3, "softplus", None, 1.0, 16)
# more slots of "another relation" than any chunk holds (positive 2's first six negatives), and one slot with both
# entities replaced: the six-row path several times per chunk
MANY_REL_CASE = ("d12-many-rel-reg", 12, 11, 7, "sigmoid", 0.5, 1.0, 17)
MANY_REL = 6
ALL_CASES = GRAD_CASES + [THRESHOLD_CASE, ADAGRAD_CASE, MANY_REL_CASE]


def case_cfg(case):
    _, D, B, K, loss, temp, regul, seed = case
    return {"model": "ComplEx", "loss": loss, "adv_temperature": temp, "regul_rate": regul, "dim": D, "batch_size": B,
            "neg_ent": K}


def build(case):
    """(tables in complex_reference.TABLES' order, (h, t, r), cfg) of a case."""
    _, D, B, K, loss, temp, regul, seed = case
    rng = np.random.default_rng(7000 + seed)
    tabs = cr.make_tables(rng, D)
    hrt = make_batch(rng, B, K, "normal")
    bh, bt, br = hrt
    if case[0] == THRESHOLD_CASE[0]:
        for x in tabs[:2]:
            x[bh[1]] *= THRESHOLD_SCALE   # positive 1's head (its negative 0 equals the positive)
    if case[0] == MANY_REL_CASE[0]:
        for k in range(MANY_REL):
            br[(k + 1) * B + 2] = (br[2] + 1) % FREE_REL
        o = B + 5   # negative 0 of positive 5: head and tail both replaced
        bh[o], bt[o] = (bh[5] + 1) % FREE_ENT, (bt[5] + 2) % FREE_ENT
    return tabs, hrt, case_cfg(case)


def as_batch(hrt):
    """The batch dict Trainer.train_one_step takes."""
    h, t, r = hrt
    return {"batch_h": h, "batch_t": t, "batch_r": r, "batch_y": np.zeros(len(h), dtype=np.float32), "mode": "normal"}


def admission(tabs, hrt, cfg):
    """The figures a case is admitted on: (bound of a gradient cell, the worst deviation of torch's float32 gradients
    from the float64 ones, (min, max) score, the largest gradient cell change when the regulariser is switched off -
    None without one, {variant: [largest gradient cell change per table]} for the two wrong models)."""
    h, t, r = hrt
    bs = cfg["batch_size"]
    _, g64, aux = cr.loss_and_grads(tabs, h, t, r, bs, cfg)
    _, g32, _ = cr.loss_and_grads(tabs, h, t, r, bs, cfg, dtype=torch.float32)
    bound = cr.grad_bound(cr.family(cfg), aux["gmax"])
    dev32 = max(float(np.abs(a - b).max()) for a, b in zip(g32, g64))
    effect = None
    if cfg["regul_rate"]:
        _, g0, _ = cr.loss_and_grads(tabs, h, t, r, bs, dict(cfg, regul_rate=0.0))
        effect = max(float(np.abs(a - b).max()) for a, b in zip(g64, g0))
    wrong = {}
    for variant in ("flip", "no_im"):
        _, gw, _ = cr.loss_and_grads(tabs, h, t, r, bs, cfg, variant=variant)
        wrong[variant] = [float(np.abs(a - b).max()) for a, b in zip(g64, gw)]
    return bound, dev32, (float(aux["s"].min()), float(aux["s"].max())), effect, wrong


def admitted(fig, cfg):
    bound, dev32, (lo, hi), effect, wrong = fig
    return (dev32 <= bound / 4 and lo <= -2 and hi >= 2 and (not cfg["regul_rate"] or effect > 20 * bound)
            and all(x > 20 * bound for v in wrong.values() for x in v))


# Adam: three steps from a given state; entity 35 appears in step 1 only (as a corrupted tail), entity 36 and relation 2
# never: their four rows and moments must stay bit-identical
# id, D, B, K, loss, adv temperature, regul_rate, lr, first step, seed
ADAM_CASES = [
    ("adam-sig-adv", 20, 11, 3, "sigmoid", 0.5, 0.0, 1e-3, 5, 21),
    ("adam-soft-reg", 12, 11, 2, "softplus", None, 1.0, 1e-3, 0, 22),
]
ADAM_STEPS = 3
ONCE_ENT = E - 2


def build_adam(case):
    """(tables, [batch per step], cfg, (m0, v0) per table, lr, steps already done)."""
    _, D, B, K, loss, temp, regul, lr, step0, seed = case
    rng = np.random.default_rng(8000 + seed)
    tabs = cr.make_tables(rng, D)
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
        else:
            m[FREE_REL] = 0
            v[FREE_REL] = 0
        m0.append(m); v0.append(v)
    return tabs, batches, case_cfg(("", D, B, K, loss, temp, regul, seed)), (m0, v0), lr, step0
