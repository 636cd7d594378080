"""Time the fused run (Trainer.run: in-kernel sampling, k_step_csr + k_apply_buf, one hipGraph per epoch) of a TransE
above dim 512 on the WN18RR-shaped synthetic graph of tools/bench_adv.py (40,943 entities, 11 relations, batch 2000,
plain MarginLoss, SGD, p 1, norm_flag on).

neg selects k_step_csr's lane groups per positive (S 1 below 12 negatives, S 2 below 24, S 4 from there). Per
(dim, neg): epochs of --steps steps are replayed until two consecutive ones agree within 1 % (clocks and caches
settle over the first seconds: the early epochs run up to a fifth slower), then the median of --runs epochs is
reported with every run, in microseconds per step, one JSON line each. --lib PATH loads another build of the library,
for A/B runs of two builds. Needs a GPU: there is no CPU path.
"""
import argparse
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
    ap.add_argument("--lib", default=None, help="another build of libputranse_hip.so (A/B runs)")
    ap.add_argument("--dims", default="768,1024")
    ap.add_argument("--negs", default="8,12,25")
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-warmup", type=int, default=60)
    ap.add_argument("--data-dir", default=os.path.join(tempfile.gettempdir(), "putranse_bench_adv_%d" % os.getuid()))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import synth_kg
    from openke import _native
    if args.lib:
        _native.use_alternative_library(args.lib)
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransE
    from openke.module.strategy import NegativeSampling

    _native.require_gpu()
    torch.cuda.set_device(0)
    path = os.path.join(args.data_dir, "wn18rr") + os.sep
    if not os.path.exists(path + "test2id.txt"):
        os.makedirs(path, exist_ok=True)
        synth_kg.write_dataset(path, *WN18RR, seed=0, ent_skew=0.5)
    bs = args.batch
    lines = []
    for D in (int(x) for x in args.dims.split(",")):
        for neg in (int(x) for x in args.negs.split(",")):
            dl = TrainDataLoader(in_path=path, batch_size=bs, threads=8, sampling_mode="normal", bern_flag=1,
                                 filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=4)
            dl.nbatches = args.steps
            torch.manual_seed(0)
            kge = TransE(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=D, p_norm=1, norm_flag=True)
            ns = NegativeSampling(model=kge, loss=MarginLoss(margin=4.0), batch_size=bs)
            tr = Trainer(model=ns, data_loader=dl, train_times=1, alpha=0.5, use_gpu=True)

            def epoch():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                tr.run()
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b) * 1000.0 / args.steps

            prev, warm = epoch(), 1
            assert tr.last_run_fused
            while warm < args.max_warmup:
                cur = epoch()
                warm += 1
                flat = abs(cur - prev) <= 0.01 * prev
                prev = cur
                if flat:
                    break
            us = [epoch() for _ in range(args.runs)]
            lines.append(json.dumps({
                "tool": "bench_fused_wide", "dim": D, "neg": neg, "batch": bs, "steps": args.steps,
                "warmup_epochs": warm, "fused_step_us": statistics.median(us), "fused_step_us_runs": us,
                "last_loss": float(tr.last_step_losses[-1])}))
            print(lines[-1], flush=True)
            del tr, ns, kge, dl
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
