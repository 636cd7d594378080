"""Generate the golden vectors of the weighted losses and Adam (tests/golden/adv_*.npz).

Needs the reference tree and oracle/_ref/Base.so:

    python tests/golden/make_golden_adv.py

Same recipe as make_golden.py (whose helpers it uses): the reference's Python package is imported from a throw-away
copy with oracle/_ref/Base.so, on CPU, one subprocess per case. Every case is the reference's own
Trainer.train_one_step on kg_small; the fixtures hold data only (configs, batches, tables, losses, optimizer state).

  adv_g*.npz  gradient cases: a few steps of SGD at lr 1, the tables recorded before and after every step, so each
              step's table delta is the reference's float32 gradient at the tables before it.
  adv_a*.npz  Adam trajectories of 10 steps: losses, batches, initial and final tables, exp_avg / exp_avg_sq after
              step 1 and at the end.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

GRAD_CASES = [
    # name, loss, adv_temperature, loss margin, p_norm, norm_flag, model margin, epsilon, sampling, dim, bs, neg,
    # seed, torch_seed, steps
    ("g1", "sigmoid", 1.0, None, 1, False, 6.0, 2.0, "cross", 16, 50, 8, 3, 41, 2),
    ("g2", "sigmoid", 0.5, None, 2, True, None, None, "normal", 8, 40, 5, 4, 42, 2),
    ("g3", "sigmoid", None, None, 1, True, 4.0, None, "normal", 8, 60, 3, 5, 43, 3),
    ("g4", "sigmoid", None, None, 2, False, None, None, "cross", 12, 30, 6, 6, 44, 4),
    ("g5", "margin", 1.0, 3.0, 1, True, None, None, "normal", 8, 50, 4, 7, 45, 2),
    ("g6", "margin", 2.0, 5.0, 2, False, 6.0, 2.0, "cross", 16, 40, 7, 8, 46, 2),
    ("g7", "margin", None, 4.0, 1, True, 5.0, None, "normal", 8, 64, 2, 9, 47, 1),
    ("g8", "margin", None, 2.0, 2, False, 3.0, 1.0, "cross", 12, 33, 5, 10, 48, 2),
]

ADAM_CASES = [
    # name, model, loss, adv_temperature, loss margin, p_norm, norm_flag, model margin, epsilon, sampling, dim, bs,
    # neg, seed, torch_seed, lr
    ("a1", "TransE", "sigmoid", 1.0, None, 1, False, 6.0, 2.0, "cross", 16, 100, 8, 11, 51, 2e-5),
    ("a2", "TransE", "margin", 1.0, 4.0, 2, True, None, None, "normal", 12, 80, 4, 12, 52, 1e-2),
    ("a3", "TransH", "margin", None, 3.0, 1, True, None, None, "normal", 10, 80, 2, 13, 53, 1e-2),
]
ADAM_STEPS = 10


def _build(model, loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed, opt, lr):
    import torch
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss, SigmoidLoss
    from openke.module.model import TransE, TransH
    from openke.module.strategy import NegativeSampling
    dl = TrainDataLoader(in_path=mg.DATASETS["small"], batch_size=bs, threads=8, sampling_mode=sampling, bern_flag=0,
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
    torch.manual_seed(tseed)
    if model == "TransE":
        kge = TransE(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=dim, p_norm=p, norm_flag=nf, margin=gamma,
                     epsilon=eps)
    else:
        kge = TransH(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=dim, p_norm=p, norm_flag=nf)
    lo = SigmoidLoss(adv_temperature=temp) if loss == "sigmoid" else MarginLoss(adv_temperature=temp, margin=lmargin)
    ns = NegativeSampling(model=kge, loss=lo, batch_size=dl.get_batch_size())
    tr = Trainer(model=ns, data_loader=dl, train_times=0, alpha=lr, use_gpu=False, opt_method=opt)
    tr.run()   # builds the optimizer (train_times=0 runs no epoch)
    return dl, kge, tr


def _tables(kge):
    return {k.split(".")[0]: v.detach().clone().numpy() for k, v in kge.state_dict().items()
            if "embeddings" in k or "norm_vector" in k}


def _next_batch(dl, sampling):
    d = dl.cross_sampling() if sampling == "cross" else dl.sampling()
    return {"h": d["batch_h"].copy(), "t": d["batch_t"].copy(), "r": d["batch_r"].copy(), "y": d["batch_y"].copy(),
            "mode": d["mode"]}, d


def _config(model, loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed):
    return dict(model=model, loss=loss, adv_temperature=np.nan if temp is None else temp,
                loss_margin=np.nan if lmargin is None else lmargin, p_norm=p, norm_flag=nf,
                model_margin=np.nan if gamma is None else gamma, epsilon=np.nan if eps is None else eps,
                sampling=sampling, dim=dim, batch_size=bs, neg_ent=neg, seed=seed, torch_seed=tseed)


def case_grad(out, name, loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed, steps):
    dl, kge, tr = _build("TransE", loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed,
                         "sgd", 1.0)
    rec = _config("TransE", loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed)
    losses, modes = [], []
    for k, v in _tables(kge).items():
        rec["s0_" + k] = v
    for s in range(steps):
        b, d = _next_batch(dl, sampling)
        for k in ("h", "t", "r"):
            rec["b%d_%s" % (s, k)] = b[k]
        modes.append(b["mode"])
        losses.append(tr.train_one_step(d))
        for k, v in _tables(kge).items():
            rec["s%d_%s" % (s + 1, k)] = v
    np.savez_compressed(out, steps=steps, lr=1.0, losses=np.array(losses, dtype=np.float64), modes=np.array(modes),
                        **rec)


def case_adam(out, name, model, loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed, lr):
    dl, kge, tr = _build(model, loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed, "adam",
                         lr)
    rec = _config(model, loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed)
    losses, modes = [], []
    for k, v in _tables(kge).items():
        rec["init_" + k] = v
    params = {k.split(".")[0]: q for k, q in kge.named_parameters() if "embeddings" in k or "norm_vector" in k}

    def state(tag):
        for k, q in params.items():
            st = tr.optimizer.state[q]
            rec["%s_m_%s" % (tag, k)] = st["exp_avg"].detach().clone().numpy()
            rec["%s_v_%s" % (tag, k)] = st["exp_avg_sq"].detach().clone().numpy()

    for s in range(ADAM_STEPS):
        b, d = _next_batch(dl, sampling)
        for k in ("h", "t", "r"):
            rec["b%d_%s" % (s, k)] = b[k]
        modes.append(b["mode"])
        losses.append(tr.train_one_step(d))
        if s == 0:
            state("step1")
            for k, v in _tables(kge).items():
                rec["step1_" + k] = v
    state("final")
    for k, v in _tables(kge).items():
        rec["final_" + k] = v
    np.savez_compressed(out, steps=ADAM_STEPS, lr=lr, losses=np.array(losses, dtype=np.float64),
                        modes=np.array(modes), **rec)


def run_case(kind, args_json, out, tmp):
    args = json.loads(args_json)
    mg._import_reference(tmp)
    mg._silence()
    {"grad": case_grad, "adam": case_adam}[kind](out, *args)


def main():
    subprocess.check_call(["make", "-C", os.path.join(mg.REPO, "oracle"), "ref"])
    tmp = tempfile.mkdtemp(prefix="refpy_")
    jobs = [("grad", list(c), "adv_%s.npz" % c[0]) for c in GRAD_CASES]
    jobs += [("adam", list(c), "adv_%s.npz" % c[0]) for c in ADAM_CASES]
    only = sys.argv[1:]
    for kind, args, fname in jobs:
        if only and not any(fname.startswith(o) for o in only):
            continue
        print("generating", fname, flush=True)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", kind, json.dumps(args),
                               os.path.join(HERE, fname), tmp])
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case(*sys.argv[2:6])
    else:
        main()
