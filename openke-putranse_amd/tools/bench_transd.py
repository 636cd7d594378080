"""Measure the TransD step (k_step_transd + the two apply passes) and its link-prediction scores against the same work
in torch ops.

Shape: an FB15K237-shaped synthetic graph (tools/synth_kg.py: 14,541 entities, 237 relations, 272,115 triples), batch
2,721, 25 negatives, bern, filter, dim 200, p 1, norm_flag, MarginLoss(4.0), SGD at lr 1 - the recipe of
examples/train_transd_FB15K237.py.

One process, device events, 20 warm-up steps, then the median of 5 runs of 100 steps of
  * k_step_transd and the apply passes (k_apply over (ent, rel), then over (ent_transfer, rel_transfer)) each on its
    own (pt_trainer_steps_timed: events around the step launch and around both apply launches of a step),
  * the whole native step as Trainer.run() drives it (GPU sampler, step, apply passes; one host synchronisation per
    run),
  * the same step in torch ops on the same device, on the same GPU-sampled batches: embedding gathers, the projection,
    F.normalize, torch.norm, the hinge, backward, torch.optim.SGD on the dense tables,
and of one block of pt_score_rows queries (256 queries, both sides) against the same scores in torch ops.
The per-kernel figures repeat ONE device batch, so every step touches the same rows: a friendlier cache state than
training's fresh batches, and since the steps train, most of that batch's pairs go inactive and stop adding rows.
The step kernel is therefore timed a second time on a model held at the initial tables (lr 0), where margin 4 keeps
every pair active: the case the atomic floor describes. The whole-step figures use fresh batches.
Atomic floor of the step kernel (arithmetic, not a measurement): (batch * neg * 2 + batch * 6) rows of dim * 4 bytes
added with float atomics, at the ~1.3 TB/s chip-wide float-atomic rate.
Prints one JSON line; --out also writes it to a file. Needs a GPU: there is no CPU path.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

FB15K237 = (14541, 237, 272115, 17535, 20466)
ATOMIC_RATE = 1.3e12   # bytes / s of float atomics chip-wide


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2721)
    ap.add_argument("--neg", type=int, default=25)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--data-dir",
                    default=os.path.join(tempfile.gettempdir(), "putranse_bench_transd_%d" % os.getuid()))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import synth_kg
    from openke import _native
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransD
    from openke.module.strategy import NegativeSampling

    _native.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    path = os.path.join(args.data_dir, "fb15k237") + os.sep
    if not os.path.exists(path + "test2id.txt"):
        os.makedirs(path, exist_ok=True)
        synth_kg.write_dataset(path, *FB15K237, seed=0, ent_skew=0.7)
    bs, neg, D, steps = args.batch, args.neg, args.dim, args.steps
    lr, margin = 1.0, 4.0
    dl = TrainDataLoader(in_path=path, batch_size=bs, threads=8, sampling_mode="normal", bern_flag=1, filter_flag=1,
                         neg_ent=neg, neg_rel=0, random_seed=4)
    dl.nbatches = steps
    E, R = dl.get_ent_tot(), dl.get_rel_tot()
    torch.manual_seed(0)
    kge = TransD(ent_tot=E, rel_tot=R, dim_e=D, dim_r=D, p_norm=1, norm_flag=True)
    init = [t.detach().clone().to(dev) for t in kge.tables() if t is not None]
    ns = NegativeSampling(model=kge, loss=MarginLoss(margin=margin), batch_size=bs)
    tr = Trainer(model=ns, data_loader=dl, train_times=1, alpha=lr, use_gpu=True, opt_method="sgd")
    L = _native.lib()

    def timed(fn, per):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / per   # us per unit

    # ---- whole native step (warm-up: one shorter run)
    dl.nbatches = args.warmup
    tr.run()
    dl.nbatches = steps
    whole = [timed(tr.run, steps) for _ in range(args.runs)]
    native_loss = float(tr.last_step_losses[-1])

    # ---- the kernels on their own, on one GPU-sampled batch
    seq = bs * (1 + neg)
    h, t, r = (torch.zeros(seq, dtype=torch.int64, device=dev) for _ in range(3))
    y = torch.zeros(seq, dtype=torch.float32, device=dev)
    sampler = dl.device_sampler()

    def sample():
        _native.check(L.pt_sampler_sample_ex(sampler, bs, neg, 0, 0, L.pt_legacy_bern(), dl.filter, _native.ptr(h),
                                             _native.ptr(t), _native.ptr(r), _native.ptr(y), _native.stream()))

    sample()
    loss_buf = torch.zeros(1, device=dev)
    ms2 = (ctypes.c_float * 2)()
    k_step, k_apply = [], []
    for i in range(args.runs + 1):
        n = args.warmup if i == 0 else steps
        _native.check(L.pt_trainer_steps_timed(tr._native, bs, neg, _native.ptr(h), _native.ptr(t), _native.ptr(r), n,
                                               _native.ptr(loss_buf), ms2, _native.stream()))
        if i:
            k_step.append(ms2[0] * 1000.0)
            k_apply.append(ms2[1] * 1000.0)

    # ---- the step kernel with every pair active: a second model at the initial tables trained at lr 0 (the tables
    # stay where margin 4 keeps every hinge open), the case the atomic floor describes
    kge0 = TransD(ent_tot=E, rel_tot=R, dim_e=D, dim_r=D, p_norm=1, norm_flag=True)
    for dst, src in zip([x for x in kge0.tables() if x is not None], init):
        dst.data.copy_(src)
    ns0 = NegativeSampling(model=kge0, loss=MarginLoss(margin=margin), batch_size=bs)
    tr0 = Trainer(model=ns0, data_loader=dl, train_times=1, alpha=0.0, use_gpu=True, opt_method="sgd")
    tr0._setup()
    k_step0 = []
    for i in range(args.runs + 1):
        n = args.warmup if i == 0 else steps
        _native.check(L.pt_trainer_steps_timed(tr0._native, bs, neg, _native.ptr(h), _native.ptr(t), _native.ptr(r),
                                               n, _native.ptr(loss_buf), ms2, _native.stream()))
        if i:
            k_step0.append(ms2[0] * 1000.0)

    # ---- the same step in torch ops
    def project(e, ep, rp):
        return F.normalize(e + (e * ep).sum(-1, keepdim=True) * rp, 2, -1)

    def distance(ent, rel, ent_t, rel_t, hh, tt, rr, head_batch=False):
        rp = F.embedding(rr, rel_t)
        hv = project(F.embedding(hh, ent), F.embedding(hh, ent_t), rp)
        tv = project(F.embedding(tt, ent), F.embedding(tt, ent_t), rp)
        hv, rv, tv = F.normalize(hv, 2, -1), F.normalize(F.embedding(rr, rel), 2, -1), F.normalize(tv, 2, -1)
        return torch.norm(hv + (rv - tv) if head_batch else (hv + rv) - tv, 1, -1)

    def active_share(tabs):
        with torch.no_grad():
            d = distance(*tabs, h, t, r)
            p, n = d[:bs].view(-1, bs).permute(1, 0), d[bs:].view(-1, bs).permute(1, 0)
            return float((p - n > -margin).float().mean())

    active_init = active_share(init)
    active_trained = active_share([x.detach() for x in kge.tables() if x is not None])
    params = [torch.nn.Parameter(x.clone()) for x in init]
    opt = torch.optim.SGD(params, lr=lr)
    last = [0.0]
    neg_margin = torch.tensor([-margin], device=dev)

    def torch_step():
        sample()
        opt.zero_grad(set_to_none=True)
        d = distance(*params, h, t, r)
        p, n = d[:bs].view(-1, bs).permute(1, 0), d[bs:].view(-1, bs).permute(1, 0)
        loss = torch.max(p - n, neg_margin).mean() + margin
        loss.backward()
        opt.step()
        last[0] = loss

    def torch_run(n):
        for _ in range(n):
            torch_step()

    torch_run(args.warmup)
    torch_us = [timed(lambda: torch_run(steps), steps) for _ in range(args.runs)]

    # ---- one block of link-prediction rows: pt_score_rows against torch ops, both sides
    nq = args.queries
    rng = np.random.default_rng(1)
    qh, qt, qr = (torch.from_numpy(rng.integers(0, hi, nq)).to(dev) for hi in (E, E, R))
    rows = torch.empty((nq, E), dtype=torch.float32, device=dev)
    desc = kge.native_desc()
    cand = torch.arange(E, device=dev)

    def native_rows():
        for side in (0, 1):
            _native.check(L.pt_score_rows(ctypes.byref(desc), side, _native.ptr(qh), _native.ptr(qt), _native.ptr(qr),
                                          nq, _native.ptr(rows), _native.stream()))

    gpu_tabs = [x.detach() for x in kge.tables() if x is not None]

    def torch_rows():
        with torch.no_grad():
            for side in (0, 1):
                for i in range(nq):   # one query's candidates at a time, as the reference Tester scores them
                    rr = qr[i].expand(E)
                    if side == 0:
                        rows[i] = distance(*gpu_tabs, cand, qt[i].expand(E), rr, True)
                    else:
                        rows[i] = distance(*gpu_tabs, qh[i].expand(E), cand, rr)

    native_rows()
    torch_rows()
    rows_native = [timed(native_rows, 1) for _ in range(args.runs)]
    rows_torch = [timed(torch_rows, 1) for _ in range(args.runs)]

    med = statistics.median
    atomic_bytes = (bs * neg * 2 + bs * 6) * D * 4
    floor_us = atomic_bytes / ATOMIC_RATE * 1e6
    res = {
        "tool": "bench_transd", "device": torch.cuda.get_device_name(0),
        "shape": {"entities": E, "relations": R, "triples": FB15K237[2], "batch": bs, "neg": neg, "dim": D,
                  "p_norm": 1, "norm_flag": True, "loss": "MarginLoss(4.0)", "opt": "sgd", "lr": lr,
                  "sampling": "normal", "bern": 1, "filter": 1},
        "steps": steps, "warmup": args.warmup, "runs": args.runs,
        "k_step_transd_us": med(k_step), "k_step_transd_us_runs": k_step,
        "k_apply_passes_us": med(k_apply), "k_apply_passes_us_runs": k_apply,
        "k_step_transd_atomic_floor_bytes": atomic_bytes,
        "k_step_transd_atomic_floor_us_at_1.3TBps": floor_us,
        "k_step_transd_all_active_us": med(k_step0), "k_step_transd_all_active_us_runs": k_step0,
        "k_step_transd_all_active_fraction_of_floor": floor_us / med(k_step0),
        "active_pairs_of_the_repeated_batch": {"initial_tables_lr0": active_init, "trained_tables": active_trained},
        "native_step_us": med(whole), "native_step_us_runs": whole,
        "torch_step_us": med(torch_us), "torch_step_us_runs": torch_us,
        "native_over_torch_speedup": med(torch_us) / med(whole),
        "score_rows_queries": nq,
        "score_rows_native_us": med(rows_native), "score_rows_native_us_runs": rows_native,
        "score_rows_torch_us": med(rows_torch), "score_rows_torch_us_runs": rows_torch,
        "score_rows_native_over_torch_speedup": med(rows_torch) / med(rows_native),
        "kernel_figures_note": "one repeated device batch (same rows every step); whole-step figures use fresh "
                               "batches; the floor assumes every (positive, negative) pair active, which the lr 0 "
                               "figure measures; the trained figure's batch has gone mostly inactive",
        "last_loss_native": native_loss, "last_loss_torch": float(last[0].detach()),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
