"""Measure the DistMult step (k_step_distmult + k_apply_adam / k_apply) against the same step in torch ops, at the
shapes of the reference's two DistMult examples on a WN18RR-shaped synthetic graph (tools/synth_kg.py: 40,943
entities, 11 relations):

  adv       examples/train_distmult_WN18_adv.py: dim 1024, batch 2000, 64 negatives, cross sampling,
            SigmoidLoss(adv_temperature=0.5), l3_regul_rate 5e-6, Adam at lr 0.002;
  softplus  examples/train_distmult_WN18.py: dim 200, batch 869, 25 negatives, normal sampling with bern,
            SoftplusLoss, regul_rate 1, Adagrad at lr 0.5.

One process, device events, 20 warm-up steps, then the median of 5 runs of 100 steps of
  * the step kernel and the apply pass each on its own (pt_trainer_steps_timed: events around both launches of a
    step; with l3_regul_rate the apply figure includes the one-block loss launch),
  * the whole native step as Trainer.run() drives it (GPU sampler, step, apply; one host synchronisation per run),
  * the same step in torch ops on the same device, on the same GPU-sampled batches: embedding gathers, products,
    logsigmoid / softplus, softmax, both regularisers, backward, torch.optim.Adam / Adagrad on the dense tables.
The per-kernel figures repeat ONE device batch (a friendlier cache state than training's fresh batches); the
whole-step figures use fresh batches. The step kernel is reported against its float-atomic floor (the batch's
corrupted rows, dim floats each, at 1.3 TB/s), the Adam pass against its six-pass HBM floor at 6.29 TB/s, the Adagrad
pass against six passes over the rows the batch touches (w, state_sum and the gradient row, read and written).
At the adv shape the Adam pass is also timed with l3_regul_rate switched off (same kernel without the L3 flag).
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

SHAPES = {
    "adv": dict(dim=1024, batch=2000, neg=64, sampling="cross", bern=0, loss="sigmoid", temp=0.5, regul=0.0, l3=5e-6,
                opt="adam", lr=0.002),
    "softplus": dict(dim=200, batch=869, neg=25, sampling="normal", bern=1, loss="softplus", temp=None, regul=1.0,
                     l3=0.0, opt="adagrad", lr=0.5),
}


def run_shape(name, S, args, path):
    import torch
    import torch.nn.functional as F

    from openke import _native
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import SigmoidLoss, SoftplusLoss
    from openke.module.model import DistMult
    from openke.module.strategy import NegativeSampling

    dev = torch.device("cuda", 0)
    bs, neg, D, steps = S["batch"], S["neg"], S["dim"], args.steps
    dl = TrainDataLoader(in_path=path, batch_size=bs, threads=8, sampling_mode=S["sampling"], bern_flag=S["bern"],
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=4)
    dl.nbatches = steps
    E, R = dl.get_ent_tot(), dl.get_rel_tot()
    torch.manual_seed(0)
    kge = DistMult(ent_tot=E, rel_tot=R, dim=D)
    ent0 = kge.ent_embeddings.weight.detach().clone().to(dev)
    rel0 = kge.rel_embeddings.weight.detach().clone().to(dev)
    loss_mod = SigmoidLoss(adv_temperature=S["temp"]) if S["loss"] == "sigmoid" else SoftplusLoss(S["temp"])
    ns = NegativeSampling(model=kge, loss=loss_mod, batch_size=bs, regul_rate=S["regul"], l3_regul_rate=S["l3"])
    tr = Trainer(model=ns, data_loader=dl, train_times=1, alpha=S["lr"], use_gpu=True, opt_method=S["opt"])
    L = _native.lib()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / steps   # us per step

    # ---- whole native step (warm-up: one shorter run)
    dl.nbatches = args.warmup
    tr.run()
    dl.nbatches = steps
    whole = [timed(tr.run) for _ in range(args.runs)]
    native_loss = float(tr.last_step_losses[-1])

    # ---- the two kernels on their own, on one GPU-sampled batch
    seq = bs * (1 + neg)
    h, t, r = (torch.zeros(seq, dtype=torch.int64, device=dev) for _ in range(3))
    y = torch.zeros(seq, dtype=torch.float32, device=dev)
    sampler = dl.device_sampler()
    flag = [0]
    cross = S["sampling"] == "cross"

    def sample():
        """The next batch in the expanded layout; returns the regulariser's batch mode (0 normal, 1 head, 2 tail)."""
        mode = 0
        if cross:
            flag[0] = 1 - flag[0]
            mode = -1 if flag[0] == 0 else 1
        _native.check(L.pt_sampler_sample_ex(sampler, bs, neg, 0, mode, L.pt_legacy_bern() if S["bern"] else 0,
                                             dl.filter, _native.ptr(h), _native.ptr(t), _native.ptr(r), _native.ptr(y),
                                             _native.stream()))
        if mode != 0:
            fixed = t if mode == -1 else h
            fixed.view(-1, bs)[1:] = fixed[:bs]
            r.view(-1, bs)[1:] = r[:bs]
        return 0 if mode == 0 else (1 if mode == -1 else 2)

    bmode = sample()
    loss_buf = torch.zeros(1, device=dev)
    ms2 = (ctypes.c_float * 2)()

    def kernels(l3):
        ns.l3_regul_rate = l3
        tr._setup()
        tr._set_regul(ns, kge, bmode)
        a, b = [], []
        for i in range(args.runs + 1):
            n = args.warmup if i == 0 else steps
            _native.check(L.pt_trainer_steps_timed(tr._native, bs, neg, _native.ptr(h), _native.ptr(t), _native.ptr(r),
                                                   n, _native.ptr(loss_buf), ms2, _native.stream()))
            if i:
                a.append(ms2[0] * 1000.0)
                b.append(ms2[1] * 1000.0)
        tr._sync_step()
        return a, b

    k_step, k_apply = kernels(S["l3"])
    k_apply_off = kernels(0.0)[1] if S["l3"] else None
    ns.l3_regul_rate = S["l3"]
    touched = int(torch.unique(torch.cat([h, t])).numel()) + int(torch.unique(r).numel())

    # ---- the same step in torch ops
    ent = torch.nn.Parameter(ent0.clone())
    rel = torch.nn.Parameter(rel0.clone())
    if S["opt"] == "adam":
        opt = torch.optim.Adam([ent, rel], lr=S["lr"])
    else:
        opt = torch.optim.Adagrad([ent, rel], lr=S["lr"])
    last = [0.0]

    def torch_step():
        m = sample()
        opt.zero_grad(set_to_none=True)
        # (as the model gathers them: the fixed side and the relation once per positive in a head / tail batch)
        hv = F.embedding(h[:bs] if m == 2 else h, ent)
        tv = F.embedding(t[:bs] if m == 1 else t, ent)
        rv = F.embedding(r[:bs] if m else r, rel)
        if m == 0:
            sc = ((hv * rv) * tv).sum(-1)
        elif m == 1:
            sc = (hv.view(-1, bs, D) * (rv * tv)).sum(-1).flatten()
        else:
            sc = ((hv * rv) * tv.view(-1, bs, D)).sum(-1).flatten()
        p, n = sc[:bs].view(-1, bs).permute(1, 0), sc[bs:].view(-1, bs).permute(1, 0)
        w = F.softmax(n * S["temp"], dim=-1).detach() if S["temp"] is not None else None
        if S["loss"] == "sigmoid":
            nl = (w * F.logsigmoid(-n)).sum(dim=-1).mean() if w is not None else F.logsigmoid(-n).mean()
            loss = -(F.logsigmoid(p).mean() + nl) / 2
        else:
            nl = (w * F.softplus(n)).sum(dim=-1).mean() if w is not None else F.softplus(n).mean()
            loss = (F.softplus(-p).mean() + nl) / 2
        if S["regul"]:
            loss = loss + S["regul"] * ((hv ** 2).mean() + (tv ** 2).mean() + (rv ** 2).mean()) / 3
        if S["l3"]:
            loss = loss + S["l3"] * (ent.norm(p=3) ** 3 + rel.norm(p=3) ** 3)
        loss.backward()
        opt.step()
        last[0] = loss

    def torch_run(n):
        for _ in range(n):
            torch_step()

    torch_us = None   # (--skip-torch: the three torch figures are written as null)
    if not args.skip_torch:
        torch_run(args.warmup)
        torch_us = [timed(lambda: torch_run(steps)) for _ in range(args.runs)]

    med = statistics.median
    hbm = 6.29e12                       # measured float4-copy bandwidth of the MI355X (bytes / s)
    atomic_bytes = bs * neg * D * 4     # the corrupted rows, added atomically
    atomic_rate = 1.3e12                # the chip's float-atomic rate
    floor_bytes = 6 * (E + R) * D * 4 if S["opt"] == "adam" else 6 * touched * D * 4
    res = {
        "shape": dict(S, entities=E, relations=R),
        "k_step_distmult_us": med(k_step), "k_step_distmult_us_runs": k_step,
        "k_step_distmult_atomic_floor_bytes": atomic_bytes,
        "k_step_distmult_atomic_floor_us_at_1.3TBps": atomic_bytes / atomic_rate * 1e6,
        "k_step_distmult_fraction_of_atomic_floor": (atomic_bytes / atomic_rate * 1e6) / med(k_step),
        "apply_us": med(k_apply), "apply_us_runs": k_apply,
        "apply_floor_bytes": floor_bytes, "apply_touched_rows": touched,
        "apply_floor_us_at_6.29TBps": floor_bytes / hbm * 1e6,
        "apply_fraction_of_floor": (floor_bytes / hbm * 1e6) / med(k_apply),
        "apply_us_l3_off": med(k_apply_off) if k_apply_off else None, "apply_us_l3_off_runs": k_apply_off,
        "native_step_us": med(whole), "native_step_us_runs": whole,
        "torch_step_us": med(torch_us) if torch_us else None, "torch_step_us_runs": torch_us,
        "native_over_torch_speedup": med(torch_us) / med(whole) if torch_us else None,
        "last_loss_native": native_loss, "last_loss_torch": float(last[0]) if torch_us else None,
    }
    del tr
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default="adv,softplus")
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
    res = {"tool": "bench_distmult", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "runs": args.runs,
           "kernel_figures_note": "one repeated device batch (same rows every step); whole-step figures use fresh "
                                  "batches"}
    for name in args.shapes.split(","):
        res[name] = run_shape(name, SHAPES[name], args, path)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
