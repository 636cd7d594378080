"""Pin tests/lp_reference.py (the float64 reference of the link-prediction scores) to the float32 CPU oracle and
to the goldens, and measure the tolerance the GPU value tests use. CPU only.

ORACLE_DEV[D] is the worst deviation of a correct float32 implementation (the oracle) from the float64 reference
at dim D; test_gpu_lp_values.py allows the kernels four times that. The table is measured here, on inputs of the
kind the GPU tests use, and never from the kernels."""
import numpy as np
import pytest

import oracle
from helpers import golden, load, pu_energy
from conftest import KG_SMALL
from lp_reference import ORACLE_DEV, lp_min64, lp_scores64, rel_err, tol

# the dims of test_gpu_lp_values.py: its dim x model matrix, its mixed call (20, 36, 64) and its chunked grid (4)
DIMS = [4, 5, 8, 12, 20, 23, 24, 36, 40, 64, 69, 100, 200, 256, 300, 512]
E_LOCAL, R_LOCAL, N_PAIRS = 333, 5, 29


def _deviation(D):
    """worst |oracle - ref64| / max(1, ref64) over model x p x norm_flag, 29 (anchor, relation) pairs of mixed
    sides each, every local entity scored"""
    worst, where = 0.0, None
    for mi, model in enumerate(("TransE", "TransH")):
        for p in (1, 2):
            for nf in (1, 0):
                rng = np.random.default_rng(1000 * D + 100 * mi + 10 * p + nf)
                ent, rel, normv = (rng.uniform(-1, 1, (n, D)).astype(np.float32) for n in (E_LOCAL, R_LOCAL, R_LOCAL))
                loc = np.arange(E_LOCAL, dtype=np.int64)
                for k in range(N_PAIRS):
                    a, r, side = int(rng.integers(E_LOCAL)), int(rng.integers(R_LOCAL)), k % 2
                    if side == 0:
                        got = oracle.score(model, p, bool(nf), "head_batch", ent, rel, normv, loc, [a], [r])
                    else:
                        got = oracle.score(model, p, bool(nf), "tail_batch", ent, rel, normv, [a], loc, [r])
                    ref = lp_scores64(model, p, nf, ent, rel, normv if model == "TransH" else None, a, r, side)
                    dev = float(rel_err(got, ref).max())
                    if dev > worst:
                        worst, where = dev, (model, p, nf)
    return worst, where


@pytest.mark.parametrize("D", DIMS)
def test_oracle_deviation_within_table(D):
    dev, where = _deviation(D)
    print("ORACLE_DEV D %d: measured %.3e at %s, table %.3e, tol %.3e" % (D, dev, where, ORACLE_DEV[D], tol(D)))
    assert dev <= ORACLE_DEV[D], (D, dev, where)
    # two float32 evaluations of one expression: a table entry far above D ulp would be a wrong reference
    assert ORACLE_DEV[D] <= (D + 16) * 2.0 ** -24, (D, ORACLE_DEV[D])


def test_keys_per_batch_accessor():
    """pt_lp_keys_per_batch (no device call): 192 MiB of float score rows, at least one key"""
    from openke import _native as n
    f = n.lib().pt_lp_keys_per_batch
    assert [f(1 << 20), f(1), f(0), f((192 << 18) - 1), f(192 << 18), f((192 << 18) + 1), f(1 << 40)] == \
        [48, 192 << 18, 192 << 18, 1, 1, 1, 1]
    assert f(40943) == (192 << 20) // (4 * 40943)


@pytest.mark.parametrize("path", golden("universes_u*.npz"), ids=lambda p: p.split("/")[-1])
def test_lp_min64_matches_oracle_energy_on_goldens(path):
    """lp_min64 over the reference's own trained universes == helpers.pu_energy (oracle scores, the reference's
    candidate order), +inf cells included."""
    z = load(path)
    model, dim, p = str(z["model"]), int(z["dim"]), int(z["p_norm"])
    kg = oracle.KG.load(KG_SMALL)
    E = kg.ent_total
    universes = [{"ent_remap": z["u%d_ent_remap" % u], "rel_remap": z["u%d_rel_remap" % u], "ent": z["u%d_ent" % u],
                  "rel": z["u%d_rel" % u], "norm": z["u%d_norm" % u] if model == "TransH" else None}
                 for u in range(int(z["n_univ"]))]
    test = oracle.sort_test(*oracle.read_triples(KG_SMALL + "test2id.txt"))
    con_h, con_t = pu_energy(E, universes, test, model, p, dim)
    n = len(test[0])
    unis64, pairs = [], []
    for u in universes:
        unis64.append({"ent": u["ent"], "rel": u["rel"], "normv": u["norm"], "remap": u["ent_remap"]})
    for ui, u in enumerate(universes):
        g2l_e = {int(g): l for l, g in enumerate(u["ent_remap"])}
        g2l_r = {int(g): l for l, g in enumerate(u["rel_remap"])}
        for q in range(n):
            h, t, r = int(test[0][q]), int(test[1][q]), int(test[2][q])
            if r not in g2l_r:
                continue
            if t in g2l_e:   # key 2q: head prediction, the anchor is the tail
                pairs.append((2 * q, ui, g2l_e[t], g2l_r[r], 0))
            if h in g2l_e:   # key 2q + 1: tail prediction
                pairs.append((2 * q + 1, ui, g2l_e[h], g2l_r[r], 1))
    rows, _ = lp_min64(unis64, pairs, E, 2 * n, model, p, True)
    worst = 0.0
    for q in range(n):
        for key, con, truth in ((2 * q, con_h[q], int(test[0][q])), (2 * q + 1, con_t[q], int(test[1][q]))):
            ref = rows[key][oracle.candidates(E, truth)]
            assert np.array_equal(np.isfinite(ref), np.isfinite(con)), (q, key)
            worst = max(worst, float(rel_err(con, ref).max()))
    print("%s: dim %d, worst oracle-vs-ref64 %.3e, tol %.3e" % (path.split("/")[-1], dim, worst, tol(dim)))
    assert worst <= tol(dim), (worst, tol(dim))
