"""The synthetic cases of tests/test_gpu_rotate.py, shared with tests/test_rotate_reference_cpu.py (which checks their
input conditions on the CPU): E = 37 entities and R = 3 relations, so rows collide constantly; batches given
explicitly (transd_cases.make_batch: entity 36 and relation 2 are never drawn - their rows must stay bit-identical -
and every batch carries the planted slots of transd_cases.plant: a positive self-loop, a negative equal to its
positive, in normal mode a negative with another relation, a positive's head equal to another positive's corrupted
entity).

Tables are at the model's init scale: entity components within +-s (gamma + eps) / (2 dim), phases within
+-(gamma + eps) / dim (phi within +-pi). At uniform(-1, 1) the relation gradient carries pi dim / (gamma + eps) and
torch's own float32 evaluation is 2-5e-5 off float64 from dim 512 up. s is chosen per case so that the distances
straddle gamma (both sigmoid branches alive), the loss margins of the MarginLoss cases so that 20-80 % of the pairs
are on the hinge's slope.

Small moduli are natural here (h == t under a small phase gives |v| = |h| 2 |sin(phi / 2)|), and a gradient element
through a small modulus is ill-conditioned in float32 whoever computes it. A case is admitted (admission(), asserted
in test_rotate_reference_cpu.py) only if four times the worst first-order conditioning estimate of any gradient cell
(rotate_reference.loss_and_grads) is within the cell's bound and torch's own float32 evaluation of the case is within
a quarter of it; the seeds below were searched on the CPU for that. No cell is exempted in the GPU tests.

What the search found, and why the tables are drawn as make_tables draws them. A relation cell is touched by every
slot of its relation (half of the batch: two relations are drawn), so its estimate is 2^-23 times the sum of
|dL/dd_k| (|h| + |t|) / |v| over those slots: about 0.25 (SigmoidLoss) or the active share (MarginLoss) times the
mean of (|h| + |t|) / |v|, which is 2.3 for independent uniform components and has a heavy tail (1 / |v| has no
variance in two dimensions). With uniform components the worst cell of 9,600-16,000 seeds per case stayed above
the bound from dim 200 up (dim 200: 5.0e-7 against 4.77e-7 under SigmoidLoss, 8.5e-7 against 8.4e-7 under MarginLoss)
and at dim 5 under MarginLoss with the adversarial weights (5.1e-7). So the tail is cut by construction instead: at
every complex element the 37 entities take 37 distinct moduli (LEVELS, a fresh permutation per element, uniform
angles), so |v| >= ||h| - |t|| > 0 between any two entities, and every phase has |phi| >= 0.16 pi, so a self-loop's
|v| = |h| 2 |sin(phi / 2)| >= 0.49 |h|. Under the adversarial weights a MarginLoss case weighs its active pairs up
(its sum is then above 1 in expectation against a bound of 4.77e-7 / 2^-21 = 1): that form is admitted at dim 5, the
larger dims run plain MarginLoss (bound 8.4e-7) and SigmoidLoss; the example's own loss runs at dim 1,024 with
K = 130. A head_batch / tail_batch case is evaluated as the models evaluate it (the fixed side and the relation
gathered once per positive): in the expanded form torch's float32 scatter of 4,847 slots into three phase rows is
itself 4.8e-7 off float64 at K = 130."""
import numpy as np
import torch

import rotate_reference as rr
from rotate_reference import E, R
from transd_cases import FREE_ENT, FREE_REL, as_batch, make_batch, planted  # noqa: F401  (re-exported)

GAMMA, EPS = 6.0, 2.0

# id, D, B, K, mode, loss, adv temperature, loss margin, table scale s, seed
GRAD_CASES = [
    ("d1-sig-adv", 1, 11, 3, "normal", "sigmoid", 2.0, None, 2.5, 1),                # VEC 1, G = 2, one idle lane
    ("d2-mar-head", 2, 11, 7, "head_batch", "margin", None, 1.0, 2.5, 102),
    ("d3-sig-tail", 3, 37, 1, "tail_batch", "sigmoid", None, None, 2.5, 3),
    ("d5-mar-adv", 5, 37, 3, "normal", "margin", 1.0, 0.5, 2.5, 1311404),
    ("d8-sig-adv-head", 8, 37, 7, "head_batch", "sigmoid", 1.0, None, 2.5, 105),     # float4, G = 2
    ("d20-mar", 20, 37, 3, "normal", "margin", None, 0.5, 2.5, 106),
    ("d200-mar-tail", 200, 37, 7, "tail_batch", "margin", None, 0.02, 2.75, 107),    # G = 64 with 14 idle lanes
    ("d260-mar", 260, 37, 3, "normal", "margin", None, 0.02, 2.75, 8),               # 2 pieces, the second 1 chunk
    ("d512-mar-head", 512, 37, 7, "head_batch", "margin", None, 0.02, 2.75, 809),    # 2 whole pieces
    ("d516-mar-tail", 516, 37, 3, "tail_batch", "margin", None, 0.02, 2.75, 810),    # 3 pieces (KCH 3)
    ("d1024-mar", 1024, 37, 7, "normal", "margin", None, 0.02, 2.75, 1511),          # the example's dim (KCH 4)
    ("d8-k70-sig-adv", 8, 11, 70, "normal", "sigmoid", 2.0, None, 2.5, 12),          # K > G: strided softmax loops
    ("d1024-k130-sig-adv-head", 1024, 37, 130, "head_batch", "sigmoid", 2.0, None, 2.75, 13),   # the example's loss
]
ADAGRAD_CASE = ("adagrad", 20, 37, 3, "normal", "margin", None, 0.5, 2.5, 214)
ALL_CASES = GRAD_CASES + [ADAGRAD_CASE]


def case_cfg(case):
    _, D, B, K, mode, loss, temp, margin, scale, seed = case
    return {"model": "RotatE", "loss": loss, "adv_temperature": temp, "loss_margin": margin, "model_margin": GAMMA,
            "epsilon": EPS, "dim": D, "batch_size": B, "neg_ent": K,
            "phase_div": rr.phase_div(rr.init_ranges(D, GAMMA, EPS)[1])}


LEVELS = 0.08 ** (1.0 - np.arange(E) / (E - 1.0))   # 37 moduli, geometric from 0.08 to 1 (ratio 1.073)
PHASE_MIN = 0.16                                      # |phi| >= 0.16 pi


def make_tables(rng, D, scale):
    """Entity element j of entity e: modulus scale * ent_range * LEVELS[perm_j(e)] (a permutation of the levels per
    element), angle uniform; phase element: +-uniform(PHASE_MIN, 1) * rel_range."""
    er, rel_r = rr.init_ranges(D, GAMMA, EPS)
    rho = np.stack([LEVELS[rng.permutation(E)] for _ in range(D)], axis=1) * (scale * er)
    theta = rng.uniform(-np.pi, np.pi, size=(E, D))
    ent = np.concatenate([rho * np.cos(theta), rho * np.sin(theta)], axis=1)
    rel = rng.choice([-1.0, 1.0], size=(R, D)) * rng.uniform(PHASE_MIN, 1.0, size=(R, D)) * rel_r
    return [ent.astype(np.float32), rel.astype(np.float32)]


def build(case):
    """(tables, (h, t, r) expanded, cfg, mode) of a case."""
    _, D, B, K, mode, loss, temp, margin, scale, seed = case
    rng = np.random.default_rng(5000 + seed)
    return make_tables(rng, D, scale), make_batch(rng, B, K, mode), case_cfg(case), mode


def admission(tabs, hrt, cfg, mode):
    """The figures a case is admitted on: (bound of a gradient cell, 4 x the worst conditioning estimate, the worst
    deviation of torch's float32 gradients from the float64 ones, share of active hinge pairs, (min, max) distance)."""
    h, t, r = hrt
    _, g64, aux = rr.loss_and_grads(tabs, h, t, r, cfg["batch_size"], cfg, mode)
    _, g32, _ = rr.loss_and_grads(tabs, h, t, r, cfg["batch_size"], cfg, mode, dtype=torch.float32)
    bound = rr.grad_bound(rr.family(cfg), aux["gmax"])
    cond = 4 * max(float(c.max()) for c in aux["cond"])
    dev32 = max(float(np.abs(a - b).max()) for a, b in zip(g32, g64))
    return bound, cond, dev32, aux["active"], (float(aux["d"].min()), float(aux["d"].max()))


# Adam: three steps from a given state; entity 35 appears in step 1 only (as a corrupted tail), entity 36 never; entity
# rows 0-34 and the relation table start with nonzero moments, entity rows 35 and 36 with zero
# id, D, B, K, loss, adv temperature, loss margin, lr, first step, seed
ADAM_CASES = [
    ("adam-sig-adv", 20, 11, 3, "sigmoid", 2.0, None, 1e-3, 5, 21),
    ("adam-mar", 12, 11, 2, "margin", None, 0.5, 1e-3, 0, 22),
]
ADAM_STEPS = 3
ONCE_ENT = E - 2


def build_adam(case):
    """(tables, [expanded batch per step], cfg, (m0, v0) per table, lr, steps already done)."""
    _, D, B, K, loss, temp, margin, lr, step0, seed = case
    rng = np.random.default_rng(6000 + seed)
    tabs = make_tables(rng, D, 2.5)
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
    cfg = case_cfg(("", D, B, K, "normal", loss, temp, margin, 2.5, seed))
    return tabs, batches, cfg, (m0, v0), lr, step0
