"""Generate the golden vectors of TransD (tests/golden/transd_*.npz).

Needs the reference tree and oracle/_ref/Base.so:

    python tests/golden/make_golden_transd.py

Same recipe as make_golden_adv.py (whose helpers it uses through make_golden.py): the reference's Python package is
imported from a throw-away copy with oracle/_ref/Base.so, on CPU, one subprocess per case. The fixtures hold data
only (configs, batches, tables, losses, optimizer state, scores, ranks).

  transd_g*.npz  gradient cases: the reference's Trainer.train_one_step under SGD at lr 1 for 2-3 steps, the four
                 tables recorded before and after every step, so each step's table delta is the reference's float32
                 gradient at the tables before it. p 1 and 2, norm_flag on and off, normal and cross sampling, both
                 init branches. The uniform init branch needs the constructor's margin and epsilon, which also switch
                 the model margin on; the case clears margin_flag after construction, so the tables are the uniform
                 branch's and the training is plain MarginLoss on the distance (recorded as margin_flag_cleared).
  transd_a*.npz  one Adam and one Adagrad trajectory of 10 steps: losses, batches, initial and final tables, the
                 optimizer state after step 1 and at the end.
  transd_p*.npz  the reference's predict in the three modes on recorded tables (one case with a model margin:
                 predict returns the distance there too).
  transd_lp.npz  the reference Tester's metrics and per-query raw / filtered ranks on kg_small with recorded tables.
"""
import ctypes
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

TABLES = ("ent_embeddings", "rel_embeddings", "ent_transfer", "rel_transfer")

GRAD_CASES = [
    # name, p_norm, norm_flag, sampling, dim, bs, neg, loss margin, model margin, epsilon, seed, torch_seed, steps
    ("g1", 1, True, "normal", 8, 50, 4, 0.2, None, None, 3, 61, 2),
    ("g2", 1, True, "cross", 16, 40, 6, 0.3, 6.0, 2.0, 4, 62, 2),
    ("g3", 1, False, "normal", 12, 60, 3, 0.3, 6.0, 2.0, 5, 63, 3),
    ("g4", 1, False, "cross", 20, 30, 5, 0.5, None, None, 6, 64, 2),
    ("g5", 2, True, "normal", 20, 50, 5, 0.1, 4.0, 1.0, 7, 65, 2),
    ("g6", 2, True, "cross", 12, 33, 4, 0.1, None, None, 8, 66, 3),
    ("g7", 2, False, "normal", 16, 64, 2, 0.1, None, None, 9, 67, 2),
    ("g8", 2, False, "cross", 8, 40, 7, 0.05, 3.0, 1.0, 10, 68, 2),
]

OPT_CASES = [
    # name, optimizer, lr, p_norm, norm_flag, sampling, dim, bs, neg, loss margin, seed, torch_seed
    ("a1", "adam", 1e-2, 1, True, "normal", 12, 80, 4, 0.3, 11, 71),
    ("a2", "adagrad", 0.1, 2, False, "cross", 16, 60, 5, 0.1, 12, 72),
]
OPT_STEPS = 10

PREDICT_CASES = [
    # name, p_norm, norm_flag, dim, model margin, epsilon, torch_seed
    ("p1", 1, True, 8, None, None, 81),
    ("p2", 1, False, 20, 5.0, 1.0, 82),
    ("p3", 2, True, 12, None, None, 83),
    ("p4", 2, False, 16, None, None, 84),
]

LP_CASE = ("lp", 1, True, 16, 91)   # name, p_norm, norm_flag, dim, torch_seed


def _model(ent, rel, dim, p, nf, gamma, eps, tseed, clear_flag):
    import torch
    from openke.module.model import TransD
    torch.manual_seed(tseed)
    kge = TransD(ent_tot=ent, rel_tot=rel, dim_e=dim, dim_r=dim, p_norm=p, norm_flag=nf, margin=gamma, epsilon=eps)
    if clear_flag:
        kge.margin_flag = False
    return kge


def _build(p, nf, sampling, dim, bs, neg, lmargin, gamma, eps, seed, tseed, opt, lr):
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.strategy import NegativeSampling
    dl = TrainDataLoader(in_path=mg.DATASETS["small"], batch_size=bs, threads=8, sampling_mode=sampling, bern_flag=0,
                         filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
    kge = _model(dl.get_ent_tot(), dl.get_rel_tot(), dim, p, nf, gamma, eps, tseed, True)
    ns = NegativeSampling(model=kge, loss=MarginLoss(margin=lmargin), batch_size=dl.get_batch_size())
    tr = Trainer(model=ns, data_loader=dl, train_times=0, alpha=lr, use_gpu=False, opt_method=opt)
    tr.run()   # builds the optimizer (train_times=0 runs no epoch)
    return dl, kge, tr


def _tables(kge):
    sd = kge.state_dict()
    return {k: sd[k + ".weight"].detach().clone().numpy() for k in TABLES}


def _next_batch(dl, sampling):
    d = dl.cross_sampling() if sampling == "cross" else dl.sampling()
    return {"h": d["batch_h"].copy(), "t": d["batch_t"].copy(), "r": d["batch_r"].copy(), "mode": d["mode"]}, d


def _config(p, nf, sampling, dim, bs, neg, lmargin, gamma, eps, seed, tseed, kge):
    return dict(model="TransD", p_norm=p, norm_flag=nf, sampling=sampling, dim=dim, batch_size=bs, neg_ent=neg,
                loss_margin=lmargin, model_margin=np.nan if gamma is None else gamma,
                epsilon=np.nan if eps is None else eps, margin_flag_cleared=int(gamma is not None), seed=seed,
                torch_seed=tseed, state_keys=np.array(sorted(kge.state_dict().keys())))


def case_grad(out, name, p, nf, sampling, dim, bs, neg, lmargin, gamma, eps, seed, tseed, steps):
    dl, kge, tr = _build(p, nf, sampling, dim, bs, neg, lmargin, gamma, eps, seed, tseed, "sgd", 1.0)
    rec = _config(p, nf, sampling, dim, bs, neg, lmargin, gamma, eps, seed, tseed, kge)
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


def case_opt(out, name, opt, lr, p, nf, sampling, dim, bs, neg, lmargin, seed, tseed):
    dl, kge, tr = _build(p, nf, sampling, dim, bs, neg, lmargin, None, None, seed, tseed, opt, lr)
    rec = _config(p, nf, sampling, dim, bs, neg, lmargin, None, None, seed, tseed, kge)
    losses, modes = [], []
    for k, v in _tables(kge).items():
        rec["init_" + k] = v
    params = {k.split(".")[0]: q for k, q in kge.named_parameters() if k.split(".")[0] in TABLES}

    def state(tag):
        for k, q in params.items():
            st = tr.optimizer.state[q]
            if opt == "adam":
                rec["%s_m_%s" % (tag, k)] = st["exp_avg"].detach().clone().numpy()
                rec["%s_v_%s" % (tag, k)] = st["exp_avg_sq"].detach().clone().numpy()
            else:
                rec["%s_sum_%s" % (tag, k)] = st["sum"].detach().clone().numpy()

    for s in range(OPT_STEPS):
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
    np.savez_compressed(out, optimizer=opt, steps=OPT_STEPS, lr=lr, losses=np.array(losses, dtype=np.float64),
                        modes=np.array(modes), **rec)


def case_predict(out, name, p, nf, dim, gamma, eps, tseed):
    import torch
    ent, rel, n = 37, 3, 29
    kge = _model(ent, rel, dim, p, nf, gamma, eps, tseed, False)
    rng = np.random.default_rng(tseed)
    rec = {}
    h, t, r = rng.integers(0, ent, n), rng.integers(0, ent, n), rng.integers(0, rel, n)
    batches = {"normal": (h, t, r), "head_batch": (rng.integers(0, ent, n), t[:1], r[:1]),
               "tail_batch": (h[:1], rng.integers(0, ent, n), r[:1])}
    for mode, (bh, bt, br) in batches.items():
        data = {"batch_h": torch.from_numpy(bh.astype(np.int64)), "batch_t": torch.from_numpy(bt.astype(np.int64)),
                "batch_r": torch.from_numpy(br.astype(np.int64)), "mode": mode}
        rec[mode + "_h"], rec[mode + "_t"], rec[mode + "_r"] = bh, bt, br
        rec[mode + "_score"] = np.asarray(kge.predict(data), dtype=np.float32)
    np.savez_compressed(out, model="TransD", p_norm=p, norm_flag=nf, dim=dim,
                        model_margin=np.nan if gamma is None else gamma, epsilon=np.nan if eps is None else eps,
                        torch_seed=tseed, **rec, **_tables(kge))


def case_lp(out, name, p, nf, dim, tseed):
    from openke.config import Tester
    from openke.data import TestDataLoader
    test_dl = TestDataLoader(mg.DATASETS["small"], "link")
    kge = _model(test_dl.get_ent_tot(), test_dl.get_rel_tot(), dim, p, nf, None, None, tseed, False)
    tester = Tester(model=kge, data_loader=test_dl, use_gpu=False)
    res = tester.run_link_prediction(type_constrain=False)
    lib = tester.lib
    names = ["l_rank", "l_filter_rank", "r_rank", "r_filter_rank"]
    acc = [ctypes.c_float.in_dll(lib, n) for n in names]
    test_dl.set_sampling_mode("link")
    n = lib.getTestTotal()
    ranks = np.zeros((len(names), n), dtype=np.int32)
    queries = np.zeros((n, 3), dtype=np.int32)
    for index, (dh, dt) in enumerate(test_dl):
        for a in acc:
            a.value = 0.0
        sh = tester.test_one_step(dh)
        lib.testHead(sh.__array_interface__["data"][0], index, 0)
        st = tester.test_one_step(dt)
        lib.testTail(st.__array_interface__["data"][0], index, 0)
        ranks[:, index] = [int(a.value) - 1 for a in acc]   # accumulated 1 + count
        queries[index] = (dh["batch_h"][0], dh["batch_t"][0], dh["batch_r"][0])
    np.savez_compressed(out, model="TransD", p_norm=p, norm_flag=nf, dim=dim, torch_seed=tseed,
                        metrics=np.array(res, dtype=np.float64), rank_names=np.array(names), ranks=ranks,
                        queries=queries, **_tables(kge))


def run_case(kind, args_json, out, tmp):
    args = json.loads(args_json)
    mg._import_reference(tmp)
    mg._silence()
    {"grad": case_grad, "opt": case_opt, "predict": case_predict, "lp": case_lp}[kind](out, *args)


def main():
    subprocess.check_call(["make", "-C", os.path.join(mg.REPO, "oracle"), "ref"])
    tmp = tempfile.mkdtemp(prefix="refpy_")
    jobs = [("grad", list(c), "transd_%s.npz" % c[0]) for c in GRAD_CASES]
    jobs += [("opt", list(c), "transd_%s.npz" % c[0]) for c in OPT_CASES]
    jobs += [("predict", list(c), "transd_%s.npz" % c[0]) for c in PREDICT_CASES]
    jobs += [("lp", list(LP_CASE), "transd_lp.npz")]
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
