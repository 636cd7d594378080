"""Plain float64 reference of the universe link-prediction scores (numpy only: no GPU, no oracle library).

pt_lp_min_scores scores every local entity of a universe as the missing side of each of its (key, universe) pairs
and MINs the score into the key's global row (Parallel_Universe_Config.py:446-642). The functions here restate
that, and the null_vector tuple score (calc_tuple_score, :378-388), in float64 from the float32 tables; nothing is
shared with the kernels or with oracle.c. tests/test_lp_reference_cpu.py pins them to the float32 CPU oracle and to
the goldens, tests/test_gpu_lp_values.py holds the kernels to them."""
import numpy as np

EPS = 1e-12   # F.normalize's clamp


def _is_transh(model):
    return model in ("TransH", 1)


def _normalize(x):
    n = np.sqrt(np.sum(x * x, axis=-1, keepdims=True))
    return x / np.maximum(n, EPS)


def _pnorm(v, p):
    return np.abs(v).sum(axis=-1) if p == 1 else np.sqrt((v * v).sum(axis=-1))


def lp_scores64(model, p, norm_flag, ent, rel, normv, anchor, r, side):
    """float64[E_local]: every row of ent scored as the missing side of (anchor, r). side 0: head prediction (the
    anchor is the tail), x + (r - a); side 1: tail prediction, (a + r) - x."""
    x = np.asarray(ent, dtype=np.float64)
    a = x[anchor]
    rr = np.asarray(rel[r], dtype=np.float64)
    if _is_transh(model):
        w = _normalize(np.asarray(normv[r], dtype=np.float64))
        a = a - (a @ w) * w
        x = x - (x @ w)[:, None] * w
    if norm_flag:
        a, x, rr = _normalize(a), _normalize(x), _normalize(rr)
    v = x + (rr - a) if side == 0 else (a + rr) - x
    return _pnorm(v, p)


def lp_tuple64(p, norm_flag, ent, rel, anchor, r, side):
    """calc_tuple_score: _calc against a zero vector on the raw anchor row (no projection, TransH included)."""
    a = np.asarray(ent[anchor], dtype=np.float64)
    rr = np.asarray(rel[r], dtype=np.float64)
    if norm_flag:
        a, rr = _normalize(a), _normalize(rr)
    return float(_pnorm(rr - a if side == 0 else a + rr, p))


def lp_min64(universes, pairs, global_E, n_keys, model="TransE", p=1, norm_flag=True):
    """(rows float64[n_keys][global_E], tuple float64[n_keys]): the elementwise MIN over the pairs (key, universe,
    anchor, rel, side) of lp_scores64 scattered through the universe's remap, and of lp_tuple64; +inf elsewhere.
    A universe is a dict of numpy arrays: ent, rel, normv (TransH), remap."""
    rows = np.full((n_keys, global_E), np.inf)
    tup = np.full(n_keys, np.inf)
    for key, u, anchor, r, side in pairs:
        U = universes[u]
        s = lp_scores64(model, p, norm_flag, U["ent"], U["rel"], U.get("normv"), anchor, r, side)
        rm = np.asarray(U["remap"])
        rows[key, rm] = np.minimum(rows[key, rm], s)
        tup[key] = min(tup[key], lp_tuple64(p, norm_flag, U["ent"], U["rel"], anchor, r, side))
    return rows, tup


# Worst |oracle - ref64| / max(1, ref64) per dim, of the float32 CPU oracle (oracle.score, head_batch and tail_batch)
# against lp_scores64 over model x p x norm_flag on uniform(-1, 1) tables (tests/test_lp_reference_cpu.py measures it
# again and asserts that it has not grown). Measured values rounded up to three digits.
ORACLE_DEV = {
    4: 5.57e-7, 5: 3.39e-7, 8: 2.76e-7, 12: 2.75e-7, 20: 3.15e-7, 23: 3.14e-7, 24: 3.40e-7, 36: 4.28e-7,
    40: 4.12e-7, 64: 5.78e-7, 69: 6.40e-7, 100: 6.25e-7, 200: 9.50e-7, 256: 1.03e-6, 300: 9.90e-7, 512: 1.38e-6,
}

TOL_FLOOR = 4 * 2.0 ** -23
TOL_CAP = 1e-5   # north_star's fp32 bound


def tol(D):
    """Relative tolerance (of max(1, ref64)) of a GPU score at dim D: four times what a second correct float32
    implementation of the same expression deviates from float64, at least 4 ulp, at most north_star's 1e-5."""
    return min(TOL_CAP, max(TOL_FLOOR, 4 * ORACLE_DEV[D]))


def rel_err(got, ref):
    """|got - ref| / max(1, ref) on the cells where ref is finite (both float64 arrays)."""
    fin = np.isfinite(ref)
    out = np.zeros(ref.shape)
    out[fin] = np.abs(np.asarray(got, dtype=np.float64)[fin] - ref[fin]) / np.maximum(1.0, ref[fin])
    return out
