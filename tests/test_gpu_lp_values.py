"""The universe link-prediction scores against a plain float64 reference, value by value (pytest -m gpu).

pt_lp_min_scores (k_lp_bases + k_lp_scan_t, planned in capi.cpp) produces the score rows behind every metric of
Parallel_Universe_Config.run_link_prediction(). The rank tests forgive near-ties and test_gpu_lp_scan.py compares
the kernel with itself; here every finite cell of the rows and of the null_vector tuple row is held to
tests/lp_reference.py: |got - ref64| <= tol(D) * max(1, ref64), tol(D) = min(1e-5, max(4 * 2^-23, 4 * ORACLE_DEV[D])),
ORACLE_DEV the deviation of a second correct float32 implementation (the CPU oracle) from the same reference,
measured by tests/test_lp_reference_cpu.py, never from the kernels. No cell is excluded; the finite mask must equal
the reference's exactly. A cell that is the MIN over universes of several dims takes the largest of their tol.

(a) dim x model x p x norm_flag on one universe: sum8's remainder / group / 16-wide loop, odd dims (the VEC = 1 bases
    kernel), the LDS opt-in from dim 256, the largest dim; tiles smaller than a wave, exact, spilling, partial.
(b) one call over 14 universes of mixed dims: several shape classes, dims sharing a class (base rows `ds` apart), a
    universe without pairs in the middle; also bit-equal to the MIN of one call per universe.
(c) four key batches (pt_lp_keys_per_batch) at global_E = 2^20, compared on the device.
(d) 65 540 active universes in one job: grid.y chunks at 65 535.
(e) argument errors leave the rows untouched."""
import ctypes

import numpy as np
import pytest
import torch

from lp_reference import lp_min64, rel_err, tol

pytestmark = pytest.mark.gpu

INF = float("inf")
MODEL_ID = {"TransE": 0, "TransH": 1}
PT_OK, PT_EINVAL, PT_ENOTSUP = 0, 1, 6   # include/putranse.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible HIP device"


def _universe(rng, D, Eu, Ru, remap, transh):
    h = {"ent": rng.uniform(-1, 1, (Eu, D)).astype(np.float32), "rel": rng.uniform(-1, 1, (Ru, D)).astype(np.float32),
         "normv": rng.uniform(-1, 1, (Ru, D)).astype(np.float32) if transh else None,
         "remap": np.asarray(remap, dtype=np.int64)}
    d = {k: torch.from_numpy(v).cuda() for k, v in h.items() if v is not None}
    return {"h": h, "d": d}


def _universe_array(n, unis):
    """pt_lp_universe[len(unis)] as rows of 7 words (ent, rel, normv, ent_total, rel_total, dim, d_ent_remap)"""
    assert ctypes.sizeof(n.LpUniverse) == 56
    a = np.zeros((len(unis), 7), dtype=np.uint64)
    for i, u in enumerate(unis):
        d = u["d"]
        a[i] = [d["ent"].data_ptr(), d["rel"].data_ptr(), d["normv"].data_ptr() if "normv" in d else 0,
                d["ent"].shape[0], d["rel"].shape[0], d["ent"].shape[1], d["remap"].data_ptr()]
    return a


def _call(n, ua, model, p, nf, pairs, E, rows, tup):
    """pt_lp_min_scores into rows / tup (device, preset to +inf); returns the status"""
    arr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 5)
    rc = n.lib().pt_lp_min_scores(ua.ctypes.data_as(ctypes.POINTER(n.LpUniverse)), len(ua), MODEL_ID[model], p, nf,
                                  arr.ctypes.data_as(ctypes.POINTER(n.LpPair)), len(arr), E, n.ptr(rows), n.ptr(tup),
                                  n.stream())
    torch.cuda.synchronize()
    return rc


def _run(n, ua, model, p, nf, pairs, E, n_keys, with_tuple=True):
    rows = torch.full((n_keys, E), INF, device="cuda")
    tup = torch.full((n_keys,), INF, device="cuda") if with_tuple else None
    n.check(_call(n, ua, model, p, nf, pairs, E, rows, tup))
    return rows, tup


def _cell_tol(unis, pairs, E, n_keys):
    """per cell the largest tol(D) among the universes whose scores the cell is the MIN of"""
    t, tt = np.zeros((n_keys, E)), np.zeros(n_keys)
    for key, u, _, _, _ in pairs:
        h = unis[u]["h"]
        x = tol(h["ent"].shape[1])
        t[key, h["remap"]] = np.maximum(t[key, h["remap"]], x)
        tt[key] = max(tt[key], x)
    return t, tt


def _check(what, got, ref, cell_tol):
    """every cell: finite exactly where the reference is (+inf elsewhere), and within its tolerance"""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "%s: finite mask differs at %d cells" % (
        what, int((np.isfinite(got) != fin).sum()))
    assert (got[~fin] == np.inf).all(), what
    err = rel_err(got, ref)
    worst = float(err.max()) if err.size else 0.0
    print("LPVAL %s worst %.3e tol %.3e" % (what, worst, float(cell_tol[fin].max()) if fin.any() else 0.0))
    bad = err > cell_tol
    assert not bad.any(), "%s: %d cells over tolerance, worst |got - ref| / max(1, ref) %.3e (tol %.3e)" % (
        what, int(bad.sum()), float(err[bad].max()), float(cell_tol[bad].min()))
    return worst


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------ (a)
DIMS_A = [5, 8, 12, 23, 24, 40, 69, 100, 200, 256, 300, 512]
E_LOCAL_A = [37, 64, 65, 333]   # a tile smaller than a wave, exactly one tile, one row of spill, a partial last tile


@pytest.mark.parametrize("p,nf", [(1, 1), (2, 1), (1, 0), (2, 0)])
@pytest.mark.parametrize("model", ["TransE", "TransH"])
@pytest.mark.parametrize("D", DIMS_A)
def test_scores_match_fp64(D, model, p, nf):
    from openke import _native as n
    case = DIMS_A.index(D) + 4 * MODEL_ID[model] + 2 * (p - 1) + (1 - nf)
    rng = np.random.default_rng(7000 + 97 * D + case)
    E, n_keys, Ru = 2000, 29, 5
    Eu = E_LOCAL_A[case % 4]   # every dim meets every count over its eight cases
    u = _universe(rng, D, Eu, Ru, np.sort(rng.choice(E, Eu, replace=False)), model == "TransH")
    # 29 pairs, distinct keys, mixed sides: 8 waves take (w, w + 8), then (w + 16, w + 24) or w + 16 alone
    keys = rng.permutation(n_keys)
    pairs = [(int(keys[k]), 0, int(rng.integers(Eu)), int(rng.integers(Ru)), int(rng.integers(2)) if k > 1 else k)
             for k in range(n_keys)]
    ua = _universe_array(n, [u])
    rows, tup = _run(n, ua, model, p, nf, pairs, E, n_keys)
    ref_rows, ref_tup = lp_min64([u["h"]], pairs, E, n_keys, model, p, nf)
    what = "a D %d %s p %d nf %d Eu %d" % (D, model, p, nf, Eu)
    _check(what + " rows", rows.cpu().numpy(), ref_rows, np.full(ref_rows.shape, tol(D)))
    _check(what + " tuple", tup.cpu().numpy(), ref_tup, np.full(ref_tup.shape, tol(D)))
    rows2, _ = _run(n, ua, model, p, nf, pairs, E, n_keys, with_tuple=False)
    assert _bits_equal(rows, rows2), what + ": rows depend on d_key_tuple"


# ------------------------------------------------------------------------------------------ (b)
DIMS_B = [8, 20, 36, 64, 40, 23, 69, 100, 200, 200, 256, 300, 512, 12]   # 36, 64, 40: one shape class, three dims
E_LOCAL_B = [30, 700, 65, 333, 64, 128, 257, 500, 100, 613, 37, 450, 191, 640]
PAIRS_B = [1, 7, 8, 9, 16, 17, 29, 0, 1, 7, 8, 9, 16, 17]   # {0, 1, 7, 8, 9, 16, 17, 29} repeated; the 0 in the middle


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("model", ["TransE", "TransH"])
def test_mixed_call_matches_fp64_and_single_universe_calls(model, p):
    from openke import _native as n
    rng = np.random.default_rng(4242 + 10 * MODEL_ID[model] + p)
    E, n_keys, nf, Ru = 4096, 40, 1, 6
    pool = np.sort(rng.choice(E, 1500, replace=False))   # remaps overlap: a pool entity sits in ~3.4 universes
    unis = [_universe(rng, D, Eu, Ru, np.sort(rng.choice(pool, Eu, replace=False)), model == "TransH")
            for D, Eu in zip(DIMS_B, E_LOCAL_B)]
    assert PAIRS_B[0] and PAIRS_B[-1] and 0 in PAIRS_B
    pairs, nxt = [], 0
    for ui, cnt in enumerate(PAIRS_B):   # keys dealt round-robin: 145 pairs, every key held by 3 or 4 universes
        for _ in range(cnt):
            key = nxt % n_keys
            nxt += 1
            pairs.append((key, ui, int(rng.integers(E_LOCAL_B[ui])), int(rng.integers(Ru)), key % 2))
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    holders = [len({u for k, u, _, _, _ in pairs if k == key}) for key in range(n_keys)]
    assert min(holders) >= 3, holders
    ua = _universe_array(n, unis)
    rows, tup = _run(n, ua, model, p, nf, pairs, E, n_keys)
    ref_rows, ref_tup = lp_min64([u["h"] for u in unis], pairs, E, n_keys, model, p, nf)
    t_rows, t_tup = _cell_tol(unis, pairs, E, n_keys)
    what = "b %s p %d" % (model, p)
    _check(what + " rows", rows.cpu().numpy(), ref_rows, t_rows)
    _check(what + " tuple", tup.cpu().numpy(), ref_tup, t_tup)
    # a pair's score does not depend on what else the call plans: the same universe array, one universe's pairs a call
    acc_r = torch.full((n_keys, E), INF, device="cuda")
    acc_t = torch.full((n_keys,), INF, device="cuda")
    for ui in range(len(unis)):
        r1, t1 = _run(n, ua, model, p, nf, [pr for pr in pairs if pr[1] == ui], E, n_keys)
        acc_r, acc_t = torch.minimum(acc_r, r1), torch.minimum(acc_t, t1)
    diff = int((rows.view(torch.int32) != acc_r.view(torch.int32)).sum())
    assert diff == 0, "%s: %d cells differ from the MIN of one call per universe" % (what, diff)
    assert _bits_equal(tup, acc_t), what + ": tuple row differs from the MIN of one call per universe"


# ------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("model,p", [("TransE", 1), ("TransH", 2)])
def test_key_batches_match_fp64(model, p):
    from openke import _native as n
    rng = np.random.default_rng(99 + p)
    E, nf, Ru = 1 << 20, 1, 4
    kpb = int(n.lib().pt_lp_keys_per_batch(E))
    assert kpb == 48   # 192 MiB of float rows of 2^20 entities
    n_keys = 3 * kpb + 5
    assert (n_keys + kpb - 1) // kpb >= 4
    dims, counts = [20, 69, 200, 200], [190, 200, 211, 205]
    unis = []
    for ui, (D, Eu) in enumerate(zip(dims, counts)):
        remap = rng.choice(np.arange(1, E - 1), Eu, replace=False)
        if ui == 3:
            remap[:2] = [0, E - 1]   # the first and the last column of a row
        unis.append(_universe(rng, D, Eu, Ru, np.sort(remap), model == "TransH"))
    key_of = rng.permutation(n_keys)   # shuffled key order
    pairs = [(int(key_of[k]), ui, int(rng.integers(counts[ui])), int(rng.integers(Ru)), int(key_of[k]) % 2)
             for ui in range(4) for k in range(n_keys) if k % 3 == ui % 3]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    assert len({k // kpb for k, _, _, _, _ in pairs}) >= 4
    # the reference over the columns any universe maps to (the others stay +inf: counted on the device below)
    cols = np.unique(np.concatenate([u["h"]["remap"] for u in unis]))
    compact = [dict(u["h"], remap=np.searchsorted(cols, u["h"]["remap"])) for u in unis]
    ref_rows, ref_tup = lp_min64(compact, pairs, len(cols), n_keys, model, p, nf)
    t_rows, t_tup = _cell_tol([{"h": c} for c in compact], pairs, len(cols), n_keys)
    ua = _universe_array(n, unis)
    rows, tup = _run(n, ua, model, p, nf, pairs, E, n_keys)   # ~600 MB: stays on the device
    got = rows[:, torch.from_numpy(cols).cuda()].cpu().numpy()
    n_finite = int(torch.isfinite(rows).sum())
    n_inf = int((rows == INF).sum())
    del rows
    what = "c %s p %d" % (model, p)
    _check(what + " rows", got, ref_rows, t_rows)
    _check(what + " tuple", tup.cpu().numpy(), ref_tup, t_tup)
    assert n_finite == int(np.isfinite(ref_rows).sum()), (n_finite, int(np.isfinite(ref_rows).sum()))
    assert n_finite + n_inf == n_keys * E


# ------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("p,nf", [(1, 1), (2, 0)])
def test_more_universes_than_one_grid(p, nf):
    """65 540 universes with a pair each in one job: k_lp_scan_t runs in grid.y chunks of 65 535 universes."""
    from openke import _native as n
    rng = np.random.default_rng(31 + p)
    NU, D, E, n_keys = 65540, 4, 512, 8
    ent = rng.uniform(-1, 1, (3 * NU, D)).astype(np.float32)   # universe u: rows 3u .. 3u + 2
    rel = rng.uniform(-1, 1, (2, D)).astype(np.float32)
    c0 = rng.integers(0, 500, NU)   # three distinct columns below 500: c0, c0 + 1..249, c0 + 250..499 (mod 500)
    remap = np.stack([c0, (c0 + rng.integers(1, 250, NU)) % 500, (c0 + rng.integers(250, 500, NU)) % 500],
                     axis=1).astype(np.int64)
    for j in range(5):   # columns 505 .. 509: each reached by one of the last five universes only
        remap[NU - 5 + j, j % 3] = 505 + j
    u_ids = np.arange(NU)
    key, anchor, r = u_ids % n_keys, rng.integers(0, 3, NU), rng.integers(0, 2, NU)
    side = key % 2
    d_ent, d_rel, d_remap = (torch.from_numpy(x).cuda() for x in (ent, rel, remap))
    ua = np.zeros((NU, 7), dtype=np.uint64)
    ua[:, 0] = d_ent.data_ptr() + u_ids * 3 * D * 4
    ua[:, 1] = d_rel.data_ptr()
    ua[:, 3], ua[:, 4], ua[:, 5] = 3, 2, D
    ua[:, 6] = d_remap.data_ptr() + u_ids * 3 * 8
    pairs = np.stack([key, u_ids, anchor, r, side], axis=1).astype(np.int32)
    rows, tup = _run(n, ua, "TransE", p, nf, pairs, E, n_keys)
    # the reference, vectorised over the universes
    x = ent.astype(np.float64).reshape(NU, 3, D)
    a, rr = x[u_ids, anchor], rel.astype(np.float64)[r]

    def unit(v):
        return v / np.maximum(np.sqrt((v * v).sum(-1, keepdims=True)), 1e-12) if nf else v

    def pnorm(v):
        return np.abs(v).sum(-1) if p == 1 else np.sqrt((v * v).sum(-1))

    xh, ah, rh = unit(x), unit(a), unit(rr)
    v = np.where(side[:, None, None] == 0, xh + (rh - ah)[:, None, :], (ah + rh)[:, None, :] - xh)
    ref_rows, ref_tup = np.full((n_keys, E), np.inf), np.full(n_keys, np.inf)
    np.minimum.at(ref_rows, (np.repeat(key, 3), remap.reshape(-1)), pnorm(v).reshape(-1))
    np.minimum.at(ref_tup, key, pnorm(np.where(side[:, None] == 0, rh - ah, ah + rh)))
    for j in range(5):   # finite only because of universe NU - 5 + j
        assert np.isfinite(ref_rows[(NU - 5 + j) % n_keys, 505 + j])
        assert not np.isfinite(np.delete(ref_rows[:, 505 + j], (NU - 5 + j) % n_keys)).any()
    what = "d p %d nf %d" % (p, nf)
    _check(what + " rows", rows.cpu().numpy(), ref_rows, np.full(ref_rows.shape, tol(D)))
    _check(what + " tuple", tup.cpu().numpy(), ref_tup, np.full(ref_tup.shape, tol(D)))


# ------------------------------------------------------------------------------------------ (e)
def test_argument_errors_leave_rows_untouched():
    from openke import _native as n
    L = n.lib()
    rng = np.random.default_rng(5)
    E, n_keys, Eu, Ru = 300, 4, 40, 3
    good = _universe(rng, 20, Eu, Ru, np.sort(rng.choice(E, Eu, replace=False)), False)
    wide = _universe(rng, 516, Eu, Ru, np.sort(rng.choice(E, Eu, replace=False)), False)
    ua = _universe_array(n, [good, wide])
    ok = (0, 0, 1, 1, 0)
    cases = [("dim 516", (1, 1, 0, 0, 1), PT_ENOTSUP, "dim not supported"),
             ("anchor = ent_total", (1, 0, Eu, 0, 0), PT_EINVAL, "local ids out of range"),
             ("rel = rel_total", (1, 0, 0, Ru, 0), PT_EINVAL, "local ids out of range"),
             ("side 2", (1, 0, 0, 0, 2), PT_EINVAL, "side must be 0 or 1"),
             ("key -1", (-1, 0, 0, 0, 0), PT_EINVAL, "key must be non-negative"),
             ("universe = n_universes", (1, 2, 0, 0, 0), PT_EINVAL, "universe out of range")]
    for what, bad, want_rc, msg in cases:
        rows = torch.full((n_keys, E), INF, device="cuda")
        tup = torch.full((n_keys,), INF, device="cuda")
        rc = _call(n, ua, "TransE", 1, 1, [ok, bad, ok], E, rows, tup)   # the bad pair between two good ones
        assert rc == want_rc, (what, rc)
        assert msg in L.pt_last_error().decode(), (what, L.pt_last_error().decode())
        assert bool((rows == INF).all()) and bool((tup == INF).all()), what + ": rows written"
    assert L.pt_lp_min_scores(None, 0, 0, 1, 1, None, 0, E, None, None, n.stream()) == PT_OK
    rows = torch.full((n_keys, E), INF, device="cuda")
    assert _call(n, ua, "TransE", 1, 1, [ok], E, rows, None) == PT_OK   # and the good pair alone does score
    assert int(torch.isfinite(rows).sum()) == Eu
