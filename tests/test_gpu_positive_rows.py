"""Stored positive rows of the large-neg TransE step (k_pos_slots, k_step_csr, k_apply_buf).

Per step, the first `cap` uses of a table row by the step's positives (an entity row as h or t, a relation row
as r) get a contribution row of their own after the negatives' bs * neg rows: k_pos_slots ranks the uses and
scans the clipped counts, the step kernel stores the positive's gradient rows there with plain stores, and the
apply pass sums a row's bucket. Uses at or beyond the cap keep the float atomics into the table's gradient row
(pt_trainer_set_positive_caps; 0 / 0 = every use atomic).

Two kinds of test:
  * the step teacher-forced against the oracle, exactly as test_gpu_parity.py checks its C2 step (loss within
    1e-5 relative, tables within helpers.assert_step_close's bound at atol 2e-6; no other tolerance): TransE at
    dims 4, 8 and 200, p_norm 1 and 2, SGD and Adagrad, caps (0, 0), (1, 1), (2, 3) - most uses overflow - and
    caps nothing reaches, on every sampling path; batches of 64-256 positives of the committed graphs, where a
    relation row is used by more positives than the apply pass streams at once (8 rows: kg_small's most frequent
    relation holds a quarter of the triples) and entity rows repeat; margin 0 over several steps, where some
    positives have no active pair and must still define their reserved rows (zeros) or the next bucket sum reads
    stale rows. Neither committed graph has a triple with h == t, so that case has no test here.
  * the slot arrays themselves (pt_trainer_positive_slots after pt_trainer_sample_csr): bucket sizes equal
    min(uses, cap), the buckets tile [bs * neg, bs * neg + stored) in row order without overlap, every stored
    destination lies inside its own row's bucket, no two uses share one, and exactly the uses beyond the cap
    are -1.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import oracle
from conftest import KG_SMALL, KG_TINY
from helpers import assert_step_close, step_noise

pytestmark = pytest.mark.gpu

THREADS = 8
PATHS = {"fused": 1, "part": 2, "twopass": 0}
NO_OVERFLOW = (4096, 4096)
CAPS = [(0, 0), (1, 1), (2, 3), NO_OVERFLOW]
# dim -> graph, batch, negatives. At p_norm 1 every (pair, component) is a sign decision that may fall within rounding
# of zero, and assert_step_close lets at most max(8, 2 %) of a table's rows meet one: dim 200 keeps bs * neg * dim
# below test_gpu_parity.py's dim-200 p = 1 case (48 * 9 * 200), still with > 8 uses of the most frequent relation
SHAPES = {4: (KG_TINY, 64, 4), 8: (KG_SMALL, 256, 5), 200: (KG_SMALL, 64, 6)}


def _teacher_forced(path_kg, dim, p, opt, bs, neg, caps, sampling, steps, margin=3.0, seed=23):
    """test_gpu_parity._teacher_forced_trainer's loop for TransE with normalization, under the given caps and
    sampling path: every step starts from the oracle's state and must equal the oracle's step. margin: one value,
    or one per step (pt_trainer_update_desc between the steps)."""
    from openke import _native
    from openke.module.model import TransE
    lr, bern, filt = (0.5 if opt == "sgd" else 0.05), 1, 1
    margins = list(margin) if isinstance(margin, (list, tuple)) else [margin] * steps
    margin = margins[0]
    L = _native.lib()
    kg = oracle.KG.load(path_kg)
    E, R = kg.ent_total, kg.rel_total
    torch.manual_seed(dim + neg)
    kge = TransE(E, R, dim=dim, p_norm=p, norm_flag=True).cuda()
    ada = opt == "adagrad"
    devt = [t for t in kge.tables()]
    dacc = [None if t is None else torch.zeros_like(t) for t in devt] if ada else [None, None, None]
    ent, rel, _ = (None if t is None else t.detach().cpu().numpy().copy() for t in devt)
    accs = [np.zeros_like(ent), np.zeros_like(rel), None] if ada else [None] * 3
    desc = kge.native_desc(_native.PT_ADAGRAD if ada else _native.PT_SGD, lr, margin, tuple(dacc))
    g, smp, tr = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    _native.check(L.pt_graph_load(path_kg.encode(), ctypes.byref(g)))
    st = oracle.GlibcRand(seed).rand_reset(THREADS)
    _native.check(L.pt_sampler_create(g, THREADS, st.ctypes.data, ctypes.byref(smp)))
    _native.check(L.pt_trainer_create(ctypes.byref(desc), ctypes.byref(tr)))
    try:
        _native.check(L.pt_trainer_set_positive_caps(tr, caps[0], caps[1]))
        _native.check(L.pt_trainer_set_sampling(tr, PATHS[sampling], 0))
        loss = torch.zeros(1, device="cuda")
        for k in range(steps):
            with torch.no_grad():
                for d_, h_ in zip(devt, (ent, rel)):
                    d_.copy_(torch.from_numpy(h_))
                for d_, h_ in zip(dacc, accs):
                    if h_ is not None:
                        d_.copy_(torch.from_numpy(h_))
            if margins[k] != margin:
                margin = margins[k]
                desc = kge.native_desc(_native.PT_ADAGRAD if ada else _native.PT_SGD, lr, margin, tuple(dacc))
                _native.check(L.pt_trainer_update_desc(tr, ctypes.byref(desc)))
            _native.check(L.pt_sampler_set_seeds(smp, st.ctypes.data))
            loss.zero_()
            _native.check(L.pt_trainer_step(tr, smp, bs, neg, bern, filt, None, None, None, _native.ptr(loss),
                                            _native.stream()))
            assert L.pt_trainer_last_path(tr) == PATHS[sampling]
            got = [devt[0].detach().cpu().numpy(), devt[1].detach().cpu().numpy()]
            got_acc = [None if t is None else t.cpu().numpy() for t in dacc]
            acc0 = [None if a is None else a.copy() for a in accs]
            tab0 = [ent.copy(), rel.copy()]
            h, t, r, _ = kg.sample(st, THREADS, bs, neg, bern, filt)
            gm = oracle.grad_mass("TransE", p, True, margin, ent, rel, None, h, t, r, bs, neg)
            want = oracle.train_step("TransE", p, True, opt, lr, margin, ent, rel, None, accs, h, t, r, bs, neg)
            assert abs(float(loss.item()) - want) <= 1e-5 * max(1.0, abs(want)), (k, float(loss.item()), want)
            for i, name in enumerate(("ent", "rel")):
                w = (ent, rel)[i]
                mask = step_noise(acc0[i], accs[i], got_acc[i]) if ada else None
                assert_step_close(got[i], w, 2e-6, mask, what="step %d %s" % (k, name), before=tab0[i],
                                  gm=gm[name], lr=lr, acc_before=acc0[i])
        nxt = np.zeros(THREADS, dtype=np.uint64)
        _native.check(L.pt_sampler_get_seeds(smp, nxt.ctypes.data))
        np.testing.assert_array_equal(nxt, st)
    finally:
        torch.cuda.synchronize()
        L.pt_trainer_free(tr)
        L.pt_sampler_free(smp)
        L.pt_graph_free(g)


def _step_cases():
    """dims x p_norm x optimizer x caps; the sampling path rotates so that every path meets every cap, dim, norm
    and optimizer."""
    out = []
    for i, (dim, p, opt, caps) in enumerate(itertools.product(sorted(SHAPES), (1, 2), ("sgd", "adagrad"), CAPS)):
        out.append((dim, p, opt, caps, sorted(PATHS)[(i + i // 4) % 3]))
    return out


@pytest.mark.parametrize("case", _step_cases(), ids=lambda c: "d%d-p%d-%s-caps%d_%d-%s" % (c[0], c[1], c[2], c[3][0],
                                                                                          c[3][1], c[4]))
def test_step_with_stored_positive_rows(case):
    dim, p, opt, caps, sampling = case
    path_kg, bs, neg = SHAPES[dim]
    _teacher_forced(path_kg, dim, p, opt, bs, neg, caps, sampling, steps=3)


@pytest.mark.parametrize("caps", [(2, 3), NO_OVERFLOW], ids=lambda c: "caps%d_%d" % c)
@pytest.mark.parametrize("dim", [4, 8])
def test_margin_zero_defines_reserved_rows(dim, caps):
    """margin 0: a positive whose negatives all score higher has no active pair; its stored rows must hold zeros,
    not the previous step's rows (six steps, so every reserved row has been written before).

    Not at dim 200: at margin 0 the decision threshold p - n = 0 sits in the middle of the score differences, and the
    oracle's near-tie window grows with the dim (2 (dim + 16) eps (|p| + |n|), oracle.c): with 64 x 6 pairs at dim
    200 it marks 30 of kg_small's 500 entity rows in the first step, and assert_step_close admits max(8, 2 %) = 10,
    so no batch of >= 64 positives can be compared there. The whole-wave lane group of dim 200 takes the zero stores
    in test_inactive_positives_define_reserved_rows below."""
    path_kg, bs, neg = SHAPES[dim]
    _teacher_forced(path_kg, dim, 2, "sgd", bs, neg, caps, "part", steps=6, margin=0.0)


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("caps", [(2, 3), NO_OVERFLOW], ids=lambda c: "caps%d_%d" % c)
def test_inactive_positives_define_reserved_rows(caps, opt):
    """dim 200 (one positive per 64-lane group): steps at margin 3 store every positive's rows; at margin -3 no pair
    of the next steps is active (p - n > 3 never holds for normalized rows at p_norm 2), so every positive returns
    early and must overwrite its reserved rows with zeros: the tables must stay where they were, as the oracle's
    do. No decision is near its threshold at either margin."""
    path_kg, bs, neg = SHAPES[200]
    _teacher_forced(path_kg, 200, 2, opt, bs, neg, caps, "fused", steps=4, margin=[3.0, -3.0, 3.0, -3.0])


class _Ctx:
    def __init__(self, seed, dim=4, path=KG_SMALL):
        from openke import _native
        _native.require_gpu()
        self.n = _native
        self.L = _native.lib()
        self.g = ctypes.c_void_p()
        _native.check(self.L.pt_graph_load(path.encode(), ctypes.byref(self.g)))
        self.E = int(self.L.pt_graph_ent_total(self.g))
        self.R = int(self.L.pt_graph_rel_total(self.g))
        st0 = oracle.GlibcRand(seed).rand_reset(THREADS)
        self.s = ctypes.c_void_p()
        _native.check(self.L.pt_sampler_create(self.g, THREADS, st0.ctypes.data, ctypes.byref(self.s)))
        dev = torch.device("cuda", 0)
        self.ent = torch.zeros(self.E, dim, device=dev)
        self.rel = torch.zeros(self.R, dim, device=dev)
        d = _native.ModelDesc()
        d.model, d.p_norm, d.norm_flag, d.opt, d.lr, d.margin = 0, 1, 1, 0, 0.1, 1.0
        d.ent_total, d.rel_total, d.dim = self.E, self.R, dim
        d.ent, d.rel = self.ent.data_ptr(), self.rel.data_ptr()
        self.t = ctypes.c_void_p()
        _native.check(self.L.pt_trainer_create(ctypes.byref(d), ctypes.byref(self.t)))

    def slots(self, bs, neg, calls, path):
        pos = np.zeros((calls, bs, 3), np.int32)
        rec = np.zeros((calls, bs * neg), np.int32)
        dst = np.zeros((calls, bs * neg), np.int32)
        start = np.zeros((calls, self.E + 1), np.int32)
        self.n.check(self.L.pt_trainer_sample_csr(self.t, self.s, bs, neg, 1, 1, calls, path, pos.ctypes.data,
                                                  rec.ctypes.data, dst.ctypes.data, start.ctypes.data,
                                                  self.n.stream()))
        pdst = np.full((calls, bs, 3), -7, np.int32)
        pstart = np.full((calls, self.E + self.R + 1), -7, np.int32)
        stored = ctypes.c_int32(-1)
        self.n.check(self.L.pt_trainer_positive_slots(self.t, calls, pdst.ctypes.data, pstart.ctypes.data,
                                                      ctypes.byref(stored), self.n.stream()))
        return pos, pdst, pstart, stored.value

    def close(self):
        self.L.pt_trainer_free(self.t)
        self.L.pt_sampler_free(self.s)
        self.L.pt_graph_free(self.g)


def _check_slots(pos, pdst, pstart, E, R, bs, neg, ent_cap, rel_cap):
    base = bs * neg
    for c in range(pos.shape[0]):
        h, r, t = pos[c, :, 0], pos[c, :, 1], pos[c, :, 2]
        uses = np.concatenate([np.bincount(h, minlength=E) + np.bincount(t, minlength=E), np.bincount(r, minlength=R)])
        size = np.minimum(uses, np.concatenate([np.full(E, ent_cap), np.full(R, rel_cap)]))
        # sizes min(uses, cap); the buckets follow one another from the end of the negatives' rows: disjoint
        np.testing.assert_array_equal(pstart[c], base + np.concatenate([[0], np.cumsum(size)]),
                                      err_msg="call %d bucket starts" % c)
        assert pstart[c, -1] <= base + 3 * bs
        row = np.stack([h, E + r, t], 1).reshape(-1)   # the row every use belongs to
        d = pdst[c].reshape(-1)
        on = d >= 0
        assert (d[~on] == -1).all()
        # every stored destination inside its own row's bucket, no destination used twice
        assert (d[on] >= pstart[c][row[on]]).all() and (d[on] < pstart[c][row[on] + 1]).all(), "call %d" % c
        assert len(np.unique(d[on])) == int(on.sum()), "call %d: a destination is used twice" % c
        # stored uses per row = the bucket's size, so exactly the uses beyond the cap are atomic
        np.testing.assert_array_equal(np.bincount(row[on], minlength=E + R), size, err_msg="call %d" % c)


@pytest.mark.parametrize("caps", [(1, 1), (2, 3), (8, 32), NO_OVERFLOW], ids=lambda c: "caps%d_%d" % c)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_slot_arrays(path, caps):
    bs, neg, calls = 200, 13, 3
    ctx = _Ctx(5)
    try:
        ctx.n.check(ctx.L.pt_trainer_set_positive_caps(ctx.t, caps[0], caps[1]))
        pos, pdst, pstart, stored = ctx.slots(bs, neg, calls, PATHS[path])
        assert stored == 1
        _check_slots(pos, pdst, pstart, ctx.E, ctx.R, bs, neg, caps[0], caps[1])
        if caps == (1, 1):   # the uses do overflow at this shape, in both tables
            assert (pdst[:, :, 1] == -1).any() and (pdst[:, :, (0, 2)] == -1).any()
        if caps == NO_OVERFLOW:
            assert (pdst >= 0).all()
    finally:
        ctx.close()


def test_caps_zero_and_library_choice():
    """0 / 0: nothing stored (also after stored caps: the arrays return to empty); -1 / -1: the library's caps,
    reported by the getter and obeyed by the slots; negative caps below -1 are refused."""
    bs, neg = 200, 13
    ctx = _Ctx(7)
    try:
        ec, rc = ctypes.c_int32(), ctypes.c_int32()
        ctx.n.check(ctx.L.pt_trainer_positive_caps(ctx.t, ctypes.byref(ec), ctypes.byref(rc)))
        assert ec.value > 0 and rc.value > 0
        pos, pdst, pstart, stored = ctx.slots(bs, neg, 2, -1)
        assert stored == 1
        _check_slots(pos, pdst, pstart, ctx.E, ctx.R, bs, neg, ec.value, rc.value)
        ctx.n.check(ctx.L.pt_trainer_set_positive_caps(ctx.t, 0, 0))
        pos, pdst, pstart, stored = ctx.slots(bs, neg, 2, -1)
        assert (pdst == -1).all() and (pstart == bs * neg).all()
        ctx.n.check(ctx.L.pt_trainer_positive_caps(ctx.t, ctypes.byref(ec), ctypes.byref(rc)))
        assert (ec.value, rc.value) == (0, 0)
        assert ctx.L.pt_trainer_set_positive_caps(ctx.t, -2, 1) != 0
    finally:
        ctx.close()


def test_nothing_stored_off_the_float4_pair():
    """dim 6 is no multiple of 4: the step runs k_step_sampled, which knows no stored rows, so none are handed out
    whatever the caps."""
    bs, neg = 100, 5
    ctx = _Ctx(9, dim=6)
    try:
        ctx.n.check(ctx.L.pt_trainer_set_positive_caps(ctx.t, 8, 32))
        pos, pdst, pstart, stored = ctx.slots(bs, neg, 2, -1)
        assert stored == 0
        assert (pdst == -1).all() and (pstart == bs * neg).all()
    finally:
        ctx.close()
