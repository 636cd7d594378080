"""Measure the self-adversarial RotatE step (k_step_rotate + k_apply_adam) against the same step in torch ops.

Shape: a WN18RR-shaped synthetic graph (tools/synth_kg.py: 40,943 entities, 11 relations), batch 2000, 64 negatives,
cross sampling, dim 1024 (entity rows of 2,048 floats), margin 6, epsilon 2, SigmoidLoss(adv_temperature=2), Adam at
lr 2e-5 - the recipe of examples/train_rotate_WN18_adv.py.

One process, device events, 20 warm-up steps, then the median of 5 runs of 100 steps of
  * k_step_rotate and k_apply_adam each on its own (pt_trainer_steps_timed: events around both launches of a step),
  * the whole native step as Trainer.run() drives it (GPU sampler, broadcast of the fixed side, step, apply; one
    host synchronisation per run),
  * the same step in torch ops on the same device, on the same GPU-sampled batches: embedding gathers, cos / sin, the
    complex product, the stacked norm, logsigmoid, softmax, backward, torch.optim.Adam on the dense tables - what a
    user would run without the kernels.
The per-kernel figures repeat ONE device batch, so every step touches the same 128,000 corrupted rows and the same
flagged rows: a friendlier cache state than training's fresh batches. The whole-step figures use fresh batches.
k_step_rotate is also reported against its float-atomic floor (the batch's corrupted rows, 2 * dim floats each, at
1.3 TB/s), k_apply_adam against its six-pass HBM floor at 6.29 TB/s.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--neg", type=int, default=64)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--data-dir", default=os.path.join(tempfile.gettempdir(), "putranse_bench_adv_%d" % os.getuid()))
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-torch", action="store_true", help="leave out the torch-op step")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F

    import synth_kg
    from openke import _native
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import SigmoidLoss
    from openke.module.model import RotatE
    from openke.module.strategy import NegativeSampling

    _native.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    path = os.path.join(args.data_dir, "wn18rr") + os.sep
    if not os.path.exists(path + "test2id.txt"):
        os.makedirs(path, exist_ok=True)
        synth_kg.write_dataset(path, *WN18RR, seed=0, ent_skew=0.5)
    bs, neg, D, steps = args.batch, args.neg, args.dim, args.steps
    lr, gamma, eps, temp = 2e-5, 6.0, 2.0, 2.0
    dl = TrainDataLoader(in_path=path, batch_size=bs, threads=8, sampling_mode="cross", bern_flag=0, filter_flag=1,
                         neg_ent=neg, neg_rel=0, random_seed=4)
    dl.nbatches = steps
    E, R = dl.get_ent_tot(), dl.get_rel_tot()
    torch.manual_seed(0)
    kge = RotatE(ent_tot=E, rel_tot=R, dim=D, margin=gamma, epsilon=eps)
    q = kge.phase_divisor()
    ent0 = kge.ent_embeddings.weight.detach().clone().to(dev)
    rel0 = kge.rel_embeddings.weight.detach().clone().to(dev)
    ns = NegativeSampling(model=kge, loss=SigmoidLoss(adv_temperature=temp), batch_size=bs, regul_rate=0.0)
    tr = Trainer(model=ns, data_loader=dl, train_times=1, alpha=lr, use_gpu=True, opt_method="adam")
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

    def sample():
        flag[0] = 1 - flag[0]
        mode = -1 if flag[0] == 0 else 1
        _native.check(L.pt_sampler_sample_ex(sampler, bs, neg, 0, mode, L.pt_legacy_bern(), dl.filter, _native.ptr(h),
                                             _native.ptr(t), _native.ptr(r), _native.ptr(y), _native.stream()))
        fixed = t if mode == -1 else h
        fixed.view(-1, bs)[1:] = fixed[:bs]
        r.view(-1, bs)[1:] = r[:bs]

    sample()
    loss_buf = torch.zeros(1, device=dev)
    ms2 = (ctypes.c_float * 2)()
    k_step, k_adam = [], []
    for i in range(args.runs + 1):
        n = args.warmup if i == 0 else steps
        _native.check(L.pt_trainer_steps_timed(tr._native, bs, neg, _native.ptr(h), _native.ptr(t), _native.ptr(r), n,
                                               _native.ptr(loss_buf), ms2, _native.stream()))
        if i:
            k_step.append(ms2[0] * 1000.0)
            k_adam.append(ms2[1] * 1000.0)

    # ---- the same step in torch ops
    ent = torch.nn.Parameter(ent0.clone())
    rel = torch.nn.Parameter(rel0.clone())
    opt = torch.optim.Adam([ent, rel], lr=lr)
    last = [0.0]

    def torch_step():
        sample()
        opt.zero_grad(set_to_none=True)
        re_h, im_h = torch.chunk(F.embedding(h, ent), 2, dim=-1)
        re_t, im_t = torch.chunk(F.embedding(t, ent), 2, dim=-1)
        phase = F.embedding(r, rel) / q
        c, s = torch.cos(phase), torch.sin(phase)
        v = torch.stack([re_h * c - im_h * s - re_t, re_h * s + im_h * c - im_t], dim=0)
        sc = gamma - v.norm(dim=0).sum(dim=-1)
        p, n = sc[:bs].view(-1, bs).permute(1, 0), sc[bs:].view(-1, bs).permute(1, 0)
        w = F.softmax(n * temp, dim=-1).detach()
        loss = -(F.logsigmoid(p).mean() + (w * F.logsigmoid(-n)).sum(dim=-1).mean()) / 2
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
    floor_bytes = 6 * (2 * E + R) * D * 4   # w, m, v read and written
    hbm = 6.29e12                           # measured float4-copy bandwidth of the MI355X (bytes / s)
    atomic_bytes = bs * neg * 2 * D * 4     # the corrupted rows (re | im), added atomically
    atomic_rate = 1.3e12                    # the chip's float-atomic rate
    res = {
        "tool": "bench_rotate", "device": torch.cuda.get_device_name(0),
        "shape": {"entities": E, "relations": R, "batch": bs, "neg": neg, "dim": D, "model_margin": gamma,
                  "epsilon": eps, "loss": "SigmoidLoss(adv_temperature=2)", "opt": "adam", "lr": lr,
                  "sampling": "cross"},
        "steps": steps, "warmup": args.warmup, "runs": args.runs,
        "k_step_rotate_us": med(k_step), "k_step_rotate_us_runs": k_step,
        "k_step_rotate_atomic_floor_bytes": atomic_bytes,
        "k_step_rotate_atomic_floor_us_at_1.3TBps": atomic_bytes / atomic_rate * 1e6,
        "k_step_rotate_fraction_of_atomic_floor": (atomic_bytes / atomic_rate * 1e6) / med(k_step),
        "k_apply_adam_us": med(k_adam), "k_apply_adam_us_runs": k_adam,
        "k_apply_adam_floor_bytes": floor_bytes,
        "k_apply_adam_floor_us_at_6.29TBps": floor_bytes / hbm * 1e6,
        "k_apply_adam_fraction_of_floor": (floor_bytes / hbm * 1e6) / med(k_adam),
        "native_step_us": med(whole), "native_step_us_runs": whole,
        "torch_step_us": med(torch_us) if torch_us else None, "torch_step_us_runs": torch_us,
        "native_over_torch_speedup": med(torch_us) / med(whole) if torch_us else None,
        "kernel_figures_note": "one repeated device batch (same rows every step); whole-step figures use fresh batches",
        "last_loss_native": native_loss, "last_loss_torch": float(last[0]) if torch_us else None,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
