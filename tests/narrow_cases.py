"""The cases of tests/test_gpu_narrow.py, shared with tests/test_narrow_reference_cpu.py, which checks their input
conditions, states which kernel instance each one selects and measures the deviation tables below on the CPU.

Two gaps of the suite are closed here:
  A. k_step_sampled (the in-kernel-sampled step of Trainer.run: every TransH model, every dim with D % 4 != 0, every
     neg_ent < 4) with k_sample_csr's batches and k_apply's contribution rows, at every (G, KCH) one-float row shape
     and every (NCH, S) column of PT_SSHAPES for both models, on kg_small batches drawn by the oracle's sampler (the
     GPU sampler is bit-exact with it), against the float64 autograd reference;
  B. the external-batch kernels and the scores at the five one-float row shapes no other test executes: (2,1,1),
     (4,1,1), (16,1,1), (64,1,4) and (64,1,8), dims 2, 3, 13, 130, 255, 257 and 511, over wide_cases' E = 70 and R = 3.

The masks of the wide one-float shapes: KCH is rounded up to a power of two, so dim 130 runs four chunks of 64 lanes
with the fourth wholly out of range, 255 four with one dead lane, 257 eight with one live lane in the fifth and three
dead chunks, 511 eight with one dead lane, 512 eight exactly full.

TransH tables whose rows would be normalised after a near-total cancellation in the projection (dims 2 and 3) are
conditioned first: see MIN_PROJECTED.

Tolerances are the project's rules (test_gpu_lp_values.py, test_gpu_adv.py, transd_reference.py) with the deviation
tables extended to these inputs by measurement on the CPU, never from the kernels:
  scores    tol(D) = min(1e-5, max(4 * 2^-23, 4 * ORACLE_DEV[D])) relative to max(1, ref64)   (TransD: SCORE_DEV[D])
  gradients min(1e-5, max(4 * 2^-23 * max(1, |g|max), 4 * GRAD_DEV_NARROW[family]))
"""
import math
import os
import re

import numpy as np
import torch

import adv_cases
import transd_cases as tc
import transd_reference as tr
import wide_cases as wc
from conftest import KG_SMALL, REPO

E, R = wc.E, wc.R
NARROW_DIMS = (2, 3, 13, 130, 255, 257, 511)   # (2,1,1) (4,1,1) (16,1,1) (64,1,4) (64,1,4) (64,1,8) (64,1,8)
TRANSD_DIMS = (13, 130, 257)

# Worst |oracle.score - lp_scores64| / max(1, ref64) per dim, measured exactly as lp_reference.ORACLE_DEV is
# (test_lp_reference_cpu._deviation), rounded up to three digits.
# Dims 2 and 3 are what TransH with norm_flag gives on unconditioned inputs (see MIN_PROJECTED): there the 1e-5 cap
# decides.
ORACLE_DEV = {2: 4.18e-4, 3: 1.03e-5, 13: 2.53e-7, 130: 8.05e-7, 255: 1.19e-6, 257: 1.14e-6, 511: 1.34e-6}

# transd_reference.measure_score_dev at the three dims, rounded up to two digits.
SCORE_DEV = {13: 2.2e-7, 130: 5.8e-7, 257: 7.4e-7}

# Worst |float32 torch autograd gradient - float64 gradient| of the reference forwards on the GPU cases' own inputs,
# per family (wide_cases.grad_dev, one thread; TransD: transd_grad_dev below), rounded up to two digits.
GRAD_DEV_NARROW = {
    "sampled_TransE": 9.2e-8,
    "sampled_TransH": 5.7e-8,
    "plain_TransE": 4.8e-7,   # p = 1 on raw rows, B = 37 / K = 7 (wide_cases.GRAD_DEV_WIDE: 3.3e-7)
    "plain_TransH": 4.2e-7,
    "sigmoid_adv": 8.9e-7,    # p = 1 on raw rows: distances of 100 to 200, whose float32 ulp the sigmoid passes on
    "sigmoid": 9.4e-10,
    "margin_adv": 3.3e-8,
    "margin_model": 2.8e-9,
    "transd_p1_raw": 4.5e-8,
    "transd_p2_norm": 4.5e-9,
    "transd_p2_raw": 6.5e-9,
}

TOL_FLOOR, TOL_CAP = wc.TOL_FLOOR, wc.TOL_CAP


def score_tol(D):
    return min(TOL_CAP, max(TOL_FLOOR, 4 * ORACLE_DEV[D]))


def transd_score_tol(D):
    return min(TOL_CAP, max(TOL_FLOOR, 4 * SCORE_DEV[D]))


def family(cfg):
    """wide_cases.family, with the sampled step's cases (section A) and TransD's in families of their own: a family's
    deviation is then never above that of the wider family it would otherwise share."""
    if cfg["model"] == "TransD":
        return "transd_" + tr.family(cfg)
    if cfg.get("sampled"):
        return "sampled_" + cfg["model"]
    return wc.family(cfg)


def grad_tol(gmax, cfg):
    return min(TOL_CAP, max(TOL_FLOOR * max(1.0, gmax), 4 * GRAD_DEV_NARROW[family(cfg)]))


def margin(p, nf, D):
    """The loss margin of a plain case: of the size of the spread of p - n on uniform(-1, 1) rows (which leaves
    between 20 % and 80 % of the pairs active), not of the distances. Raw rows: v has unit variance per component, so
    d is about sqrt(D) with a spread of order 1 under p = 2 and about 0.77 D with a spread of order sqrt(D) under
    p = 1; normalised rows divide both by about sqrt(D / 3)."""
    s = {(2, False): 0.3, (1, False): 0.3 * math.sqrt(D), (2, True): 0.5 / math.sqrt(D), (1, True): 0.4}[(p, bool(nf))]
    return float("%.2g" % s)


# ---------------------------------------------------------------------------------------- TransH at dims 2 and 3
# TransH projects e onto the relation's hyperplane, e - (e . w) w, and under norm_flag normalises the result. The
# projection carries an absolute rounding error of about 3 * 2^-24 |e| per component in any float32 evaluation (the
# dot product, its product with w, the subtraction); the normalisation divides it by |e_perp|. At dim 2 the hyperplane
# is a line and share = |e_perp| / |e| = |sin(e, w)| has its density at 0: over a few hundred (entity, relation) pairs
# of uniform rows the smallest share is about 1e-3, and the CPU oracle itself is then 4e-4 (dim 2) and 1e-5 (dim 3)
# off float64 (ORACLE_DEV above). No float32 kernel can be held to float64 on such rows, so:
#   * the score and link-prediction tables of TransH redraw every entity row whose share against any relation is under
#     MIN_PROJECTED. A score holds two such rows (anchor and candidate) and under p = 1 sums D components, so its error
#     is about 2 * sqrt(D) * 3 * 2^-24 / share: 4e-6 at dim 2 and 5e-6 at dim 3 for share = 1 / 8, half of the 1e-5
#     cap. From dim 13 on no row is ever redrawn;
#   * the gradient cases assert the same share for the rows their batches name, and leave TransH with norm_flag at dim
#     2 out: every normalised projected row is +-u there (u the unit vector of the line), its normalize Jacobian maps
#     any gradient onto w and the projection maps that to zero, so an entity's gradient through its own row is exactly
#     0 and what a float32 evaluation returns is the rounding of |g| / share (up to 2e-5 in torch's float32 autograd
#     over forty seeds): there is nothing to compare. TransH at dim 2 trains raw rows in this file.
MIN_PROJECTED = 0.125


def projected_shares(ent, normv):
    """[entities][relations] |e - (e . w^) w^| / |e| in float64."""
    e = np.asarray(ent, dtype=np.float64)
    w = np.asarray(normv, dtype=np.float64)
    w = w / np.maximum(np.sqrt((w * w).sum(-1, keepdims=True)), 1e-12)
    e2 = (e * e).sum(-1)[:, None]
    return np.sqrt(np.maximum(e2 - (e @ w.T) ** 2, 0.0) / e2)


def projected_share(ent, normv, ents=None, rels=None):
    """The smallest share over the given entities x relations (all by default)."""
    sh = projected_shares(ent, normv)
    sh = sh if ents is None else sh[np.unique(ents)]
    return float((sh if rels is None else sh[:, np.unique(rels)]).min())


def well_conditioned(model, nf, tabs, ents=None, rels=None):
    return not (model == "TransH" and nf) or projected_share(tabs[0], tabs[2], ents, rels) >= MIN_PROJECTED


def redraw_ill_conditioned(rng, ent, normv):
    """Entity rows with a share under MIN_PROJECTED against some relation, drawn again (uniform(-1, 1)) until none is
    left; returns how many draws that took."""
    n = 0
    while True:
        bad = np.nonzero(projected_shares(ent, normv).min(-1) < MIN_PROJECTED)[0]
        if not bad.size:
            return n
        ent[bad] = rng.uniform(-1, 1, size=(bad.size, ent.shape[1])).astype(np.float32)
        n += bad.size


# ---------------------------------------------------------------------------------------- B. scores
def score_case(model, D, p, nf):
    """Tables and the three modes' batches (as predict takes them) of the score tests: wide_cases.score_case over
    conditioned TransH tables."""
    rng = np.random.default_rng(8000 + 10 * D + 4 * (model == "TransH") + 2 * p + int(nf))
    tabs = adv_cases.make_tables(rng, D, 1.0, ent=E, rel=R, transh=model == "TransH")
    n = 41
    h, t, r = rng.integers(0, E, n), rng.integers(0, E, n), rng.integers(0, R, n)
    batches = {"normal": (h, t, r), "head_batch": (rng.integers(0, E, n), t[:1], r[:1]),
               "tail_batch": (h[:1], rng.integers(0, E, n), r[:1])}
    if model == "TransH":
        redraw_ill_conditioned(rng, tabs[0], tabs[2])
    return tabs, batches


LP_GLOBAL_E, LP_KEYS, LP_E_LOCAL, LP_R_LOCAL = 2000, 29, 65, 5


def lp_case(model, D, p, nf):
    """One universe (arrays ent, rel, normv or None, remap into LP_GLOBAL_E columns) of LP_E_LOCAL entities - one full
    tile of 64 and one row of spill - and 29 (key, universe, anchor, relation, side) pairs with distinct keys and
    mixed sides, as test_gpu_lp_values.test_scores_match_fp64 builds them, over conditioned TransH tables."""
    rng = np.random.default_rng(7000 + 97 * D + 4 * (model == "TransH") + 2 * (p - 1) + (1 - int(nf)))
    Eu, Ru = LP_E_LOCAL, LP_R_LOCAL
    u = {"ent": rng.uniform(-1, 1, (Eu, D)).astype(np.float32), "rel": rng.uniform(-1, 1, (Ru, D)).astype(np.float32),
         "normv": rng.uniform(-1, 1, (Ru, D)).astype(np.float32) if model == "TransH" else None,
         "remap": np.sort(rng.choice(LP_GLOBAL_E, Eu, replace=False)).astype(np.int64)}
    keys = rng.permutation(LP_KEYS)
    pairs = [(int(keys[k]), 0, int(rng.integers(Eu)), int(rng.integers(Ru)), int(rng.integers(2)) if k > 1 else k)
             for k in range(LP_KEYS)]
    if model == "TransH":
        redraw_ill_conditioned(rng, u["ent"], u["normv"])
    return u, pairs


# ---------------------------------------------------------------------------------------- kernel selection
# What launch_step (csrc/step.hip) and pt_trainer_step (csrc/trainer.cpp) select for an in-kernel-sampled step,
# restated: a statement of which instance a case runs, not a test of the launcher.
def pick_shape(D, vec4=True):
    """kernels.h pick_shape: (G, VEC, KCH)."""
    vec = 4 if vec4 and D % 4 == 0 else 1
    chunks = D // vec
    G = 1
    while G < chunks and G < 64:
        G <<= 1
    G = max(G, 2)
    kch = (chunks + G - 1) // G
    if vec == 1:
        k = 1
        while k < kch:
            k <<= 1
        kch = k
    return G, vec, kch


def pick_nch(neg, kch):
    """step.hip pick_nch: negative rows held in registers per chunk."""
    best = 1
    for o in (1, 4, 8, 32):
        if o * kch > 128:
            break
        best = o
        if o >= neg:
            break
    return best


def sshapes():
    """The (G, VEC, KCH, NCH, S) list of PT_SSHAPES, read from csrc/step.hip."""
    src = open(os.path.join(REPO, "openke-putranse_amd", "csrc", "step.hip")).read()
    body = re.search(r"#define PT_SSHAPES\(X\)(.*?)\n\s*\n", src, re.S).group(1)
    return [tuple(int(x) for x in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+)\)", body)]


def uses_csr(neg):
    """trainer.cpp use_csr: the counting-sort sampler (k_sample_csr and its LDS forms) from 4 negatives."""
    return neg >= 4


def reaches_sampled(model, D, neg):
    """Whether an in-kernel-sampled step runs k_step_sampled: not TransE with float4 rows on a counting-sort batch
    (k_step_csr, step.hip csr_fast_path)."""
    return not (uses_csr(neg) and model == "TransE" and D % 4 == 0) and 1 <= D <= 512


def sampled_instance(model, D, neg, listed=None):
    """(G, VEC, KCH, NCH, S, CSR) of the k_step_sampled instance launch_step launches: the one-float shape, S = 4 from
    8 negatives, the preferred chunk depth first and then launch_step's fallback order among the listed instances."""
    listed = sshapes() if listed is None else listed
    assert reaches_sampled(model, D, neg)
    G, vec, kch = pick_shape(D, False)
    S = 4 if neg >= 8 and 256 // G >= 4 else 1
    nper = (neg + S - 1) // S
    for nch in (pick_nch(nper, kch * vec), 8, 4, 32, 1):
        if (G, vec, kch, nch, S) in listed:
            return G, vec, kch, nch, S, uses_csr(neg)
    return None


# ---------------------------------------------------------------------------------------- A. the sampled step
# model, dim, p, norm_flag, opt, bs, neg, bern, filter, steps. One teacher-forced step per `steps` on kg_small (500
# entities, 7 relations), tables uniform(-1, 1).
SAMPLED_CASES = [
    # ---- TransE, D % 4 != 0 (and dim 300 with neg < 4)
    ("TransE", 2, 2, True, "sgd", 40, 3, 1, 1, 1),          # (2,1,1), NCH 4
    ("TransE", 3, 1, True, "sgd", 24, 8, 1, 1, 2),          # (4,1,1): 16 positives per block, 8 inactive; S = 4
    ("TransE", 7, 2, False, "adagrad", 40, 9, 1, 1, 1),     # (8,1,1), S = 4 with an empty sub-group
    ("TransE", 13, 2, False, "adagrad", 6, 140, 1, 1, 1),   # (16,1,1): sub-groups of 35 over NCH 32
    ("TransE", 23, 1, True, "sgd", 48, 1, 0, 0, 1),         # (32,1,1), NCH 1
    ("TransE", 50, 2, True, "adagrad", 40, 6, 1, 1, 1),     # (64,1,1), NCH 8, counting sort
    ("TransE", 85, 2, False, "sgd", 32, 12, 1, 1, 1),       # (64,1,2), S = 4
    ("TransE", 130, 2, True, "sgd", 40, 6, 1, 1, 2),        # (64,1,4): the fourth chunk dead; NCH 8, counting sort
    ("TransE", 130, 2, False, "adagrad", 48, 1, 1, 1, 1),   # NCH 1, no counting sort
    ("TransE", 130, 1, False, "sgd", 16, 8, 1, 1, 1),       # S = 4, two per sub-group: (64,1,4,4,4)
    ("TransE", 130, 2, True, "sgd", 8, 40, 0, 1, 1),        # sub-groups of 10: (64,1,4,32,4)
    ("TransE", 255, 1, False, "adagrad", 32, 9, 1, 1, 1),   # one dead lane; sub-groups of 3, 3, 3, 0
    ("TransE", 255, 2, True, "sgd", 40, 3, 1, 1, 1),        # NCH 4 with a partial chunk
    ("TransE", 255, 2, False, "sgd", 24, 10, 1, 0, 1),      # sub-groups of 3, 3, 3, 1
    ("TransE", 257, 2, False, "sgd", 24, 10, 1, 1, 2),      # (64,1,8): one live lane in chunk five, three dead chunks
    ("TransE", 257, 1, False, "adagrad", 32, 1, 1, 1, 1),
    ("TransE", 257, 2, True, "sgd", 40, 6, 1, 1, 1),        # NCH 8, counting sort, S = 1
    ("TransE", 511, 2, True, "adagrad", 40, 3, 1, 1, 1),    # one dead lane in chunk eight
    ("TransE", 511, 2, False, "sgd", 24, 9, 1, 1, 1),       # an empty sub-group
    ("TransE", 511, 2, True, "sgd", 12, 40, 1, 1, 1),       # sub-groups of 10 over NCH 8: two passes, the second short
    ("TransE", 300, 2, True, "sgd", 40, 2, 1, 1, 1),        # D % 4 == 0 but neg < 4
    # ---- TransH, every dim
    ("TransH", 2, 2, False, "sgd", 40, 8, 1, 1, 1),         # (2,1,1): 32 positives per block, 24 inactive in the last
    ("TransH", 3, 2, False, "adagrad", 40, 3, 1, 1, 1),
    ("TransH", 7, 2, True, "sgd", 40, 2, 0, 1, 1),
    ("TransH", 13, 2, True, "sgd", 12, 36, 1, 1, 1),        # sub-groups of 9 over NCH 32
    ("TransH", 23, 2, True, "adagrad", 40, 5, 1, 1, 1),
    ("TransH", 50, 2, False, "sgd", 10, 33, 1, 1, 1),
    ("TransH", 85, 1, False, "sgd", 48, 1, 1, 1, 1),
    ("TransH", 130, 2, False, "sgd", 24, 8, 1, 1, 2),       # the aW row of the LDS meet, raw rows
    ("TransH", 200, 2, True, "adagrad", 24, 10, 1, 1, 1),   # D % 4 == 0: (64,1,4) all the same
    ("TransH", 200, 2, False, "sgd", 40, 6, 1, 1, 1),
    ("TransH", 255, 2, True, "sgd", 48, 1, 1, 1, 1),
    ("TransH", 257, 1, False, "adagrad", 16, 9, 1, 1, 1),   # p = 1, an empty sub-group
    ("TransH", 257, 2, True, "sgd", 40, 1, 1, 0, 1),
    ("TransH", 511, 2, True, "sgd", 24, 8, 1, 1, 1),        # normalised rows through the meet
    ("TransH", 512, 2, False, "adagrad", 40, 3, 1, 1, 1),   # (64,1,8) exactly full
    ("TransH", 512, 2, True, "sgd", 8, 40, 1, 1, 2),        # two passes per sub-group
]
SAMPLER_THREADS = 8
# sampler / table seeds under which the input conditions hold (test_narrow_reference_cpu.py); every other case uses 1
SAMPLED_SEEDS = {"TransE-d130-p2-nf-sgd-bs8-neg40": 2}


def sampled_name(case):
    model, D, p, nf, opt, bs, neg = case[:7]
    return "%s-d%d-p%d-%s-%s-bs%d-neg%d" % (model, D, p, "nf" if nf else "raw", opt, bs, neg)


def sampled_cfg(case):
    model, D, p, nf, opt, bs, neg = case[:7]
    return dict(wc.plain_cfg((sampled_name(case), model, D, bs, neg, nf, p, opt, margin(p, nf, D))), sampled=True)


_SAMPLED = {}


def build_sampled(case, seed=None):
    """A sampled case's inputs and float64 reference, computed once: tables (ent, rel, norm_vector or None) over
    kg_small's entities and relations, the sampler streams before every step and after the last, each step's batch
    (the oracle's sampling() in the expanded layout) with its float64 loss, gradients and conditions."""
    import oracle
    name = sampled_name(case)
    key = (name, seed)
    if key in _SAMPLED:
        return _SAMPLED[key]
    model, D, p, nf, opt, bs, neg, bern, filt, steps = case
    s = SAMPLED_SEEDS.get(name, 1) if seed is None else seed
    kg = oracle.KG.load(KG_SMALL)
    rng = np.random.default_rng(4000 + s)
    tabs = adv_cases.make_tables(rng, D, 1.0, ent=kg.ent_total, rel=kg.rel_total, transh=model == "TransH")
    if model == "TransH" and nf:
        redraw_ill_conditioned(rng, tabs[0], tabs[2])
    cfg = sampled_cfg(case)
    st = oracle.GlibcRand(s).rand_reset(SAMPLER_THREADS)
    states, out = [], []
    for _ in range(steps):
        states.append(st.copy())
        h, t, r, _ = kg.sample(st, SAMPLER_THREADS, bs, neg, bern, filt)
        loss, grads, aux = wc.conditions(tabs, h, t, r, bs, cfg)
        out.append({"hrt": (h, t, r), "loss": loss, "grads": grads, "aux": aux})
    states.append(st.copy())
    res = {"name": name, "tabs": tabs, "cfg": cfg, "states": states, "steps": out}
    if seed is None:
        _SAMPLED[key] = res
    return res


def adagrad_state(tabs):
    """The given state_sum in [1, 2) of the Adagrad cases: |d delta / d g| <= 1 there."""
    rng = np.random.default_rng(77)
    return [None if x is None else rng.uniform(1, 2, size=x.shape).astype(np.float32) for x in tabs]


def adagrad_delta(state, g):
    return g / (np.sqrt(state.astype(np.float64) + g ** 2) + 1e-10)


# ---------------------------------------------------------------------------------------- B. the plain step
def _plain_cases():
    out = []
    for D in NARROW_DIMS:
        for model in ("TransE", "TransH"):
            for p in (1, 2):
                for opt in ("sgd", "adagrad"):
                    # (TransH at dim 2 trains raw rows only: see MIN_PROJECTED)
                    nf = (opt == "sgd") == (model == "TransE") and not (model == "TransH" and D == 2)
                    # p = 1 with normalised rows keeps to the small batch (wide_cases._plain_cases)
                    small = nf if p == 1 else not nf
                    B, K = (11, 3) if small else (37, 7)
                    name = "%s-d%d-p%d-%s-%s-b%d" % (model, D, p, "nf" if nf else "raw", opt, B)
                    out.append((name, model, D, B, K, nf, p, opt, margin(p, nf, D)))
    return out


PLAIN_CASES = _plain_cases()
PLAIN_SEEDS = {"TransH-d511-p1-raw-sgd-b37": 2}


def build_plain(case):
    """(tables, (h, t, r) expanded, cfg) of a plain-step case (wide_cases.build_plain with this file's seeds)."""
    name, model, D, B, K, nf, p, opt, m = case
    rng = np.random.default_rng(5000 + PLAIN_SEEDS.get(name, 1))
    tabs = adv_cases.make_tables(rng, D, 1.0, ent=E, rel=R, transh=model == "TransH")
    hrt = wc.make_plain_batch(rng, B, K)
    if model == "TransH" and nf:
        redraw_ill_conditioned(rng, tabs[0], tabs[2])
    return tabs, hrt, wc.plain_cfg(case)


# ---------------------------------------------------------------------------------------- B. the weighted step
# adv_cases.GRAD_CASES' four families at dims 130 and 257, each with K = 3 and K = 70 (TransE; adv_cases' tuple):
# id, D, B, K, mode, norm_flag, p, loss, adv_temperature, loss margin, model margin, table scale, seed.
# The p = 1 case keeps to raw rows, its model margin of the size of the distances (0.77 D), its temperature of the size
# of the inverse of their spread (wide_cases._adv_cases).
ADV_SEEDS = {}


def _adv_cases():
    out = []
    for D in (130, 257):
        for K in (3, 70):
            B = 37 if K == 3 else 11
            rows = [
                ("d%d-sigmoid-k%d-tail" % (D, K), D, 11, K, "tail_batch", True, 2, "sigmoid", None, None, 6.0, 1.0),
                ("d%d-sigmoid-adv-p1-k%d" % (D, K), D, 11, K, "normal", False, 1, "sigmoid", 0.1, None,
                 round(0.77 * D), 1.0),
                ("d%d-margin-adv-k%d-head" % (D, K), D, B, K, "head_batch", False, 2, "margin", 2.0,
                 margin(2, False, D), None, 1.0),
                ("d%d-margin-model-k%d" % (D, K), D, B, K, "normal", True, 2, "margin", None, margin(2, True, D), 5.0,
                 1.0),
            ]
            out += [c + (ADV_SEEDS.get(c[0], 1),) for c in rows]
    return out


ADV_CASES = _adv_cases()

# adv_cases.ADAM_CASES' two three-step cases at dims 13, 130 and 257 (wide_cases.build_adam's tuple):
# id, model, D, B, K, norm_flag, p, loss, adv_temperature, loss margin, model margin, lr, first step, seed
ADAM_SEEDS = {}
ADAM_CASES = [c + (ADAM_SEEDS.get(c[0], 1),) for D in (13, 130, 257) for c in (
    ("adam-transe-d%d" % D, "TransE", D, 11, 3, True, 2, "sigmoid", 1.0, None, 6.0, 1e-3, 5),
    ("adam-transh-d%d" % D, "TransH", D, 37, 7, True, 2, "margin", None, margin(2, True, D), None, 1e-3, 0),
)]

# ---------------------------------------------------------------------------------------- B. TransD
# one SGD gradient case per dim (transd_cases' tuple): id, D, B, K, mode, norm_flag, p, loss margin, table scale, seed
TRANSD_CASES = [
    ("transd-d13-p2", 13, 37, 3, "normal", True, 2, 0.05, 1.0, 1),
    ("transd-d130-p1-raw-tail", 130, 11, 3, "tail_batch", False, 1, 0.2, 1.0, 1),
    ("transd-d257-p2-raw-head", 257, 11, 7, "head_batch", False, 2, 0.01, 1.0, 1),
]


def transd_grads32(tabs, h, t, r, bs, cfg, mode):
    """The gradients of transd_reference's forward and loss evaluated in float32 by torch autograd on one thread."""
    tt = [torch.tensor(np.asarray(x, dtype=np.float32), requires_grad=True) for x in tabs]
    hh, t_, rr = (torch.as_tensor(np.asarray(x, dtype=np.int64)) for x in (h, t, r))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        d = tr.distances(tt, hh, t_, rr, cfg, mode)[0]
        p = d[:bs].view(-1, bs).permute(1, 0)
        n = d[bs:].view(-1, bs).permute(1, 0)
        m = float(cfg["loss_margin"])
        (torch.max(p - n, torch.tensor(-m, dtype=torch.float32)).mean() + m).backward()
    finally:
        torch.set_num_threads(threads)
    return [x.grad.numpy().astype(np.float64) for x in tt]


def transd_grad_dev(tabs, h, t, r, bs, cfg, mode):
    _, g64, _ = tr.loss_and_grads(tabs, h, t, r, bs, cfg, mode)
    g32 = transd_grads32(tabs, h, t, r, bs, cfg, mode)
    return max(float(np.abs(a - b).max()) for a, b in zip(g32, g64))


# ---------------------------------------------------------------------------------------- deviations
def gradient_inputs():
    """Every (family, name, deviation thunk) the GPU gradient and Adam tests of this file run."""
    for case in SAMPLED_CASES:
        b = build_sampled(case)
        tabs = b["tabs"]
        for k, s in enumerate(b["steps"]):
            yield (family(b["cfg"]), "%s-step%d" % (b["name"], k),
                   lambda tabs=tabs, s=s, b=b: wc.grad_dev(tabs, *s["hrt"], b["cfg"]["batch_size"], b["cfg"]))
    for case in PLAIN_CASES:
        tabs, hrt, cfg = build_plain(case)
        yield family(cfg), case[0], lambda a=(tabs, hrt, cfg): wc.grad_dev(a[0], *a[1], a[2]["batch_size"], a[2])
    for case in ADV_CASES:
        tabs, batch, cfg = wc.build_adv(case)
        hrt = wc.expanded(batch, cfg["batch_size"])
        yield family(cfg), case[0], lambda a=(tabs, hrt, cfg): wc.grad_dev(a[0], *a[1], a[2]["batch_size"], a[2])
    for case in ADAM_CASES:
        tabs, batches, cfg, _, _, _ = wc.build_adam(case)
        for s, b in enumerate(batches):
            hrt = wc.expanded(b, cfg["batch_size"])
            yield (family(cfg), "%s-step%d" % (case[0], s),
                   lambda a=(tabs, hrt, cfg): wc.grad_dev(a[0], *a[1], a[2]["batch_size"], a[2]))
    for case in TRANSD_CASES:
        tabs, hrt, cfg, mode = tc.build(case)
        yield (family(cfg), case[0],
               lambda a=(tabs, hrt, cfg, mode): transd_grad_dev(a[0], *a[1], a[2]["batch_size"], a[2], a[3]))
