"""Measure the ComplEx step (k_step_complex + both k_apply launches) against the same step in torch ops, and its
link-prediction scores, at the shape of the reference's examples/train_complex_WN18.py on a WN18RR-shaped synthetic
graph (tools/synth_kg.py: 40,943 entities, 11 relations): dim 200, batch 869 (nbatches 100), 25 negatives, normal
sampling with bern, SoftplusLoss, regul_rate 1, Adagrad at lr 0.5.

One process, device events, 20 warm-up steps, then the median of 5 runs of 100 steps of
  * the step kernel and the two apply launches (re tables, im tables) each on its own (pt_trainer_steps_timed: events
    around the step launch and around both apply launches of a step),
  * the whole native step as Trainer.run() drives it (GPU sampler, step, apply twice; one host synchronisation per run),
  * the same step in torch ops on the same device, on the same GPU-sampled batches: embedding gathers of the four
    tables, the four products, softplus, the regulariser, backward, torch.optim.Adagrad on the dense tables.
The per-kernel figures repeat ONE device batch (a friendlier cache state than training's fresh batches); the
whole-step figures use fresh batches. The step kernel is reported against its float-atomic floor (the batch's
corrupted rows, 2 * dim floats each, at 1.3 TB/s), the Adagrad passes against six passes over the rows the batch
touches in the four tables (w, state_sum and the gradient row, read and written).
Link prediction: pt_score_queries for 256 queries (both sides) over all 40,943 entities at dim 200, median of 5 runs of
10 launches per side; the figure is per launch of 256 queries.
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

WN18RR = (40943, 11, 86835, 3034, 3134)

SHAPE = dict(dim=200, batch=869, neg=25, sampling="normal", bern=1, loss="softplus", temp=None, regul=1.0,
             opt="adagrad", lr=0.5)
LP_QUERIES, LP_LAUNCHES = 256, 10


def run_shape(S, args, path):
    import torch
    import torch.nn.functional as F

    from openke import _native
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import SoftplusLoss
    from openke.module.model import ComplEx
    from openke.module.strategy import NegativeSampling

    dev = torch.device("cuda", 0)
    bs, neg, D, steps = S["batch"], S["neg"], S["dim"], args.steps
    dl = TrainDataLoader(in_path=path, batch_size=bs, threads=8, sampling_mode=S["sampling"], bern_flag=S["bern"],
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=4)
    dl.nbatches = steps
    E, R = dl.get_ent_tot(), dl.get_rel_tot()
    torch.manual_seed(0)
    kge = ComplEx(ent_tot=E, rel_tot=R, dim=D)
    names = ("ent_re_embeddings", "ent_im_embeddings", "rel_re_embeddings", "rel_im_embeddings")
    init = [getattr(kge, k).weight.detach().clone().to(dev) for k in names]
    ns = NegativeSampling(model=kge, loss=SoftplusLoss(S["temp"]), batch_size=bs, regul_rate=S["regul"])
    tr = Trainer(model=ns, data_loader=dl, train_times=1, alpha=S["lr"], use_gpu=True, opt_method=S["opt"])
    L = _native.lib()

    def timed(fn, per=steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / per   # us per step (or per launch)

    # ---- whole native step (warm-up: one shorter run)
    dl.nbatches = args.warmup
    tr.run()
    dl.nbatches = steps
    whole = [timed(tr.run) for _ in range(args.runs)]
    native_loss = float(tr.last_step_losses[-1])

    # ---- the kernels on their own, on one GPU-sampled batch
    seq = bs * (1 + neg)
    h, t, r = (torch.zeros(seq, dtype=torch.int64, device=dev) for _ in range(3))
    y = torch.zeros(seq, dtype=torch.float32, device=dev)
    sampler = dl.device_sampler()

    def sample():
        _native.check(L.pt_sampler_sample_ex(sampler, bs, neg, 0, 0, L.pt_legacy_bern() if S["bern"] else 0,
                                             dl.filter, _native.ptr(h), _native.ptr(t), _native.ptr(r), _native.ptr(y),
                                             _native.stream()))

    sample()
    loss_buf = torch.zeros(1, device=dev)
    ms2 = (ctypes.c_float * 2)()
    tr._setup()
    k_step, k_apply = [], []
    for i in range(args.runs + 1):
        n = args.warmup if i == 0 else steps
        _native.check(L.pt_trainer_steps_timed(tr._native, bs, neg, _native.ptr(h), _native.ptr(t), _native.ptr(r), n,
                                               _native.ptr(loss_buf), ms2, _native.stream()))
        if i:
            k_step.append(ms2[0] * 1000.0)
            k_apply.append(ms2[1] * 1000.0)
    touched = int(torch.unique(torch.cat([h, t])).numel()) + int(torch.unique(r).numel())

    # ---- link prediction: 256 queries over every entity, both sides
    qh, qt = (torch.randint(0, E, (LP_QUERIES,), device=dev) for _ in range(2))
    qr = torch.randint(0, R, (LP_QUERIES,), device=dev)
    rows = torch.empty(LP_QUERIES, E, dtype=torch.float32, device=dev)
    desc = kge.native_desc()

    def lp(side):
        for _ in range(LP_LAUNCHES):
            _native.check(L.pt_score_queries(ctypes.byref(desc), side, _native.ptr(qh), _native.ptr(qt),
                                             _native.ptr(qr), LP_QUERIES, _native.ptr(rows), _native.stream()))

    lp_us = {}
    for side in (0, 1):
        lp(side)
        lp_us[side] = [timed(lambda: lp(side), LP_LAUNCHES) for _ in range(args.runs)]

    # ---- the same step in torch ops
    ent_re, ent_im, rel_re, rel_im = (torch.nn.Parameter(x.clone()) for x in init)
    opt = torch.optim.Adagrad([ent_re, ent_im, rel_re, rel_im], lr=S["lr"])
    last = [0.0]

    def torch_step():
        sample()
        opt.zero_grad(set_to_none=True)
        h_re, h_im = F.embedding(h, ent_re), F.embedding(h, ent_im)
        t_re, t_im = F.embedding(t, ent_re), F.embedding(t, ent_im)
        r_re, r_im = F.embedding(r, rel_re), F.embedding(r, rel_im)
        sc = torch.sum(h_re * t_re * r_re + h_im * t_im * r_re + h_re * t_im * r_im - h_im * t_re * r_im, -1)
        p, n = sc[:bs].view(-1, bs).permute(1, 0), sc[bs:].view(-1, bs).permute(1, 0)
        loss = (F.softplus(-p).mean() + F.softplus(n).mean()) / 2
        if S["regul"]:
            loss = loss + S["regul"] * sum(torch.mean(x ** 2) for x in (h_re, h_im, t_re, t_im, r_re, r_im)) / 6
        loss.backward()
        opt.step()
        last[0] = loss

    def torch_run(n):
        for _ in range(n):
            torch_step()

    torch_us = None   # (--skip-torch: the torch figures are written as null)
    if not args.skip_torch:
        torch_run(args.warmup)
        torch_us = [timed(lambda: torch_run(steps)) for _ in range(args.runs)]

    med = statistics.median
    hbm = 6.29e12                          # measured float4-copy bandwidth of the MI355X (bytes / s)
    atomic_bytes = bs * neg * 2 * D * 4    # the corrupted rows (re and im), added atomically
    atomic_rate = 1.3e12                   # the chip's float-atomic rate
    floor_bytes = 6 * touched * 2 * D * 4
    lp_bytes = 2 * E * D * 4 + LP_QUERIES * E * 4   # both entity tables read once, the score rows written
    res = {
        "shape": dict(S, entities=E, relations=R),
        "k_step_complex_us": med(k_step), "k_step_complex_us_runs": k_step,
        "k_step_complex_atomic_floor_bytes": atomic_bytes,
        "k_step_complex_atomic_floor_us_at_1.3TBps": atomic_bytes / atomic_rate * 1e6,
        "k_step_complex_fraction_of_atomic_floor": (atomic_bytes / atomic_rate * 1e6) / med(k_step),
        "apply_both_us": med(k_apply), "apply_both_us_runs": k_apply,
        "apply_floor_bytes": floor_bytes, "apply_touched_rows": touched,
        "apply_floor_us_at_6.29TBps": floor_bytes / hbm * 1e6,
        "apply_fraction_of_floor": (floor_bytes / hbm * 1e6) / med(k_apply),
        "native_step_us": med(whole), "native_step_us_runs": whole,
        "torch_step_us": med(torch_us) if torch_us else None, "torch_step_us_runs": torch_us,
        "native_over_torch_speedup": med(torch_us) / med(whole) if torch_us else None,
        "last_loss_native": native_loss, "last_loss_torch": float(last[0]) if torch_us else None,
        "lp_256_queries_head_us": med(lp_us[0]), "lp_256_queries_head_us_runs": lp_us[0],
        "lp_256_queries_tail_us": med(lp_us[1]), "lp_256_queries_tail_us_runs": lp_us[1],
        "lp_floor_bytes": lp_bytes, "lp_floor_us_at_6.29TBps": lp_bytes / hbm * 1e6,
    }
    del tr
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--data-dir", default=os.path.join(tempfile.gettempdir(), "putranse_bench_adv_%d" % os.getuid()))
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the torch-op step")
    args = ap.parse_args()

    import torch

    import synth_kg
    from openke import _native

    _native.require_gpu()
    torch.cuda.set_device(0)
    path = os.path.join(args.data_dir, "wn18rr") + os.sep
    if not os.path.exists(path + "test2id.txt"):
        os.makedirs(path, exist_ok=True)
        synth_kg.write_dataset(path, *WN18RR, seed=0, ent_skew=0.5)
    res = {"tool": "bench_complex", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "runs": args.runs,
           "kernel_figures_note": "one repeated device batch (same rows every step); whole-step figures use fresh "
                                  "batches"}
    res["softplus"] = run_shape(SHAPE, args, path)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
