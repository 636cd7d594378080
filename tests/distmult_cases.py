"""The synthetic cases of tests/test_gpu_distmult.py, shared with tests/test_distmult_reference_cpu.py (which checks
their input conditions on the CPU): E = 37 entities and R = 3 relations, so rows collide constantly; batches given
explicitly (transd_cases.make_batch: entity 36 and relation 2 are never drawn, and every batch carries the planted
slots of transd_cases.plant: a positive self-loop, a negative equal to its positive, in normal mode a negative with
another relation, a positive's head equal to another positive's corrupted entity).

Tables are uniform(+-a) with a = sqrt(3) (1.5 / sqrt(dim))^(1/3) (distmult_reference.table_scale): the scores then have
a standard deviation near 1.5 and span about -7..+8, both sigmoid branches alive, |g|max below 1.

A case is admitted (admission(), asserted in test_distmult_reference_cpu.py) only if
  - torch's own float32 gradients of the case are within a quarter of the cell bound of the float64 ones;
  - the scores span at least [-2, 2];
  - with a regulariser, some gradient cell moves by more than 20 times its bound when the regulariser is switched off
    in the reference: a kernel that ignores the term cannot pass. regul_rate = 1 (the example's rate) does that;
    l3_regul_rate at the example's 5e-6 does not, so the L3 cases use 1e-2.
No cell is exempted in the GPU tests. The rows no batch names (entity 36, relation 2) move under L3 and under nothing
else. The seeds of d1-sig-adv, d8-k70-sig-adv and the threshold case were searched on the CPU for these
conditions (the first seeds tried spanned [-1.5, 1.4], sat at 0.49 of the bound in torch's float32, and stayed below 20)."""
import numpy as np
import torch

import distmult_reference as dr
from distmult_reference import E, R
from transd_cases import FREE_ENT, FREE_REL, as_batch, make_batch, planted  # noqa: F401  (re-exported)

# id, D, B, K, mode, loss, adv temperature, regul_rate, seed
GRAD_CASES = [
    ("d1-sig-adv", 1, 11, 3, "normal", "sigmoid", 0.5, 0.0, 101),                # VEC 1, G = 2, one idle lane
    ("d2-soft-head-reg", 2, 11, 7, "head_batch", "softplus", None, 1.0, 2),
    ("d3-sig-tail", 3, 37, 1, "tail_batch", "sigmoid", None, 0.0, 3),
    ("d5-soft-adv-reg", 5, 37, 3, "normal", "softplus", 1.0, 1.0, 4),
    ("d8-sig-adv-head", 8, 37, 7, "head_batch", "sigmoid", 0.5, 0.0, 5),         # float4, G = 2
    ("d20-soft-tail-reg", 20, 37, 3, "tail_batch", "softplus", None, 1.0, 6),
    ("d200-soft-reg", 200, 37, 7, "normal", "softplus", None, 1.0, 7),           # the example's dim; 14 idle lanes
    ("d260-sig", 260, 37, 3, "normal", "sigmoid", None, 0.0, 8),                 # 2 pieces, the second 1 chunk
    ("d512-sig-adv-head-reg", 512, 37, 7, "head_batch", "sigmoid", 0.5, 1.0, 9),  # 2 whole pieces
    ("d516-soft-tail", 516, 37, 3, "tail_batch", "softplus", None, 0.0, 10),     # 3 pieces
    ("d1024-sig-adv-reg", 1024, 37, 7, "normal", "sigmoid", 0.5, 1.0, 11),       # the example's dim: 4 pieces
    ("d8-k70-sig-adv", 8, 11, 70, "normal", "sigmoid", 0.5, 0.0, 100),           # K > G: strided softmax loops
    ("d1024-k130-sig-adv-head", 1024, 37, 130, "head_batch", "sigmoid", 0.5, 0.0, 13),
    ("d20-tail-reg-k70", 20, 11, 70, "tail_batch", "sigmoid", 1.0, 1.0, 14),
]
# an entity row scaled so that some score exceeds 20: nn.Softplus's threshold branch
THRESHOLD_CASE = ("d20-soft-threshold", 20, 11, 3, "normal", "softplus", None, 0.0, 101)
THRESHOLD_SCALE = 12.0
ADAGRAD_CASE = ("adagrad-reg", 20, 37, 3, "normal", "softplus", None, 1.0, 16)
ALL_CASES = GRAD_CASES + [THRESHOLD_CASE, ADAGRAD_CASE]

L3_RATE = 1e-2


def case_cfg(case):
    _, D, B, K, mode, loss, temp, regul, seed = case
    return {"model": "DistMult", "loss": loss, "adv_temperature": temp, "regul_rate": regul, "l3_regul_rate": 0.0,
            "dim": D, "batch_size": B, "neg_ent": K}


def make_tables(rng, D):
    a = dr.table_scale(D)
    return [rng.uniform(-a, a, size=(E, D)).astype(np.float32), rng.uniform(-a, a, size=(R, D)).astype(np.float32)]


def build(case):
    """(tables, (h, t, r) expanded, cfg, mode) of a case."""
    _, D, B, K, mode, loss, temp, regul, seed = case
    rng = np.random.default_rng(7000 + seed)
    tabs = make_tables(rng, D)
    hrt = make_batch(rng, B, K, mode)
    if case[0] == THRESHOLD_CASE[0]:
        tabs[0][hrt[0][1]] *= THRESHOLD_SCALE   # positive 1's head (its negative 0 equals the positive)
    return tabs, hrt, case_cfg(case), mode


def admission(tabs, hrt, cfg, mode):
    """The figures a case is admitted on: (bound of a gradient cell, the worst deviation of torch's float32 gradients
    from the float64 ones, (min, max) score, the largest gradient cell change when the regularisers are switched off
    - None without one)."""
    h, t, r = hrt
    bs = cfg["batch_size"]
    _, g64, aux = dr.loss_and_grads(tabs, h, t, r, bs, cfg, mode)
    _, g32, _ = dr.loss_and_grads(tabs, h, t, r, bs, cfg, mode, dtype=torch.float32)
    bound = dr.grad_bound(dr.family(cfg), aux["gmax"])
    dev32 = max(float(np.abs(a - b).max()) for a, b in zip(g32, g64))
    effect = None
    if cfg["regul_rate"] or cfg["l3_regul_rate"]:
        off = dict(cfg, regul_rate=0.0, l3_regul_rate=0.0)
        _, g0, _ = dr.loss_and_grads(tabs, h, t, r, bs, off, mode)
        effect = max(float(np.abs(a - b).max()) for a, b in zip(g64, g0))
    return bound, dev32, (float(aux["s"].min()), float(aux["s"].max())), effect


# Adam with L3: three steps from a given state; entity 35 appears in step 1 only (as a corrupted tail), entity 36 and
# relation 2 never: they start with zero moments and move by exactly what L3 alone gives them
# id, D, B, K, loss, adv temperature, regul_rate, l3_regul_rate, lr, first step, seed
ADAM_CASES = [
    ("adam-sig-adv-l3", 20, 11, 3, "sigmoid", 0.5, 0.0, L3_RATE, 1e-3, 5, 21),
    ("adam-soft-reg-l3", 12, 11, 2, "softplus", None, 1.0, L3_RATE, 1e-3, 0, 22),
    ("adam-sig-plain", 12, 11, 2, "sigmoid", None, 0.0, 0.0, 1e-3, 0, 23),   # L3 off: the free rows stay bit-identical
]
ADAM_STEPS = 3
ONCE_ENT = E - 2


def build_adam(case):
    """(tables, [expanded batch per step], cfg, (m0, v0) per table, lr, steps already done)."""
    _, D, B, K, loss, temp, regul, l3, lr, step0, seed = case
    rng = np.random.default_rng(8000 + seed)
    tabs = make_tables(rng, D)
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
    cfg = dict(case_cfg(("", D, B, K, "normal", loss, temp, regul, seed)), l3_regul_rate=l3)
    return tabs, batches, cfg, (m0, v0), lr, step0
