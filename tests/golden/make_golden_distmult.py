"""Generate the golden vectors of DistMult (tests/golden/distmult_*.npz).

Needs the reference tree and oracle/_ref/Base.so:

    python tests/golden/make_golden_distmult.py

Same recipe as make_golden_rotate.py (whose helpers it uses through make_golden.py): the reference's Python package is
imported from a throw-away copy with oracle/_ref/Base.so, on CPU, one subprocess per case. The fixtures hold data
only (configs, batches, tables, losses, optimizer state, scores, ranks).

  distmult_g*.npz  gradient cases: the reference's Trainer.train_one_step under SGD at lr 1 for 2-3 steps, both tables
                   recorded before and after every step, so each step's table delta is the reference's float32
                   gradient at the tables before it. SigmoidLoss and SoftplusLoss, each with and without the
                   adversarial weights, normal and cross sampling, regul_rate 0 and 1, dims 5 (odd), 7, 8, 12, 16, 20.
  distmult_a*.npz  one Adam trajectory with l3_regul_rate and one Adagrad trajectory with regul_rate, 10 steps each:
                   losses, batches, initial and final tables, the optimizer state after step 1 and at the end.
  distmult_p*.npz  the reference's predict (-score) in the three modes on recorded tables.
  distmult_lp.npz  the reference Tester's metrics and per-query raw / filtered ranks on kg_small with recorded tables.
Every file records state_keys (the model's state_dict keys) and the initial tables of its seeded construction; the
cases cover both init branches of the constructor (xavier; uniform when margin and epsilon are given).
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

TABLES = ("ent_embeddings", "rel_embeddings")

GRAD_CASES = [
    # name, loss, adv_temperature, regul_rate, model margin, epsilon, sampling, dim, bs, neg, seed, torch_seed, steps
    ("g1", "sigmoid", 0.5, 0.0, None, None, "cross", 8, 50, 4, 3, 261, 2),
    ("g2", "softplus", None, 1.0, None, None, "normal", 5, 40, 6, 4, 262, 3),
    ("g3", "softplus", 1.0, 1.0, 24.0, 2.0, "cross", 12, 60, 3, 5, 263, 2),
    ("g4", "sigmoid", None, 0.0, 12.0, 2.0, "normal", 7, 30, 5, 6, 264, 2),
    ("g5", "sigmoid", 1.0, 1.0, None, None, "normal", 20, 50, 5, 7, 265, 2),
    ("g6", "softplus", None, 0.0, None, None, "cross", 16, 33, 4, 8, 266, 3),
]

OPT_CASES = [
    # name, optimizer, lr, loss, adv_temperature, regul_rate, l3_regul_rate, model margin, epsilon, sampling, bern, dim,
    # bs, neg, seed, torch_seed
    ("a1", "adam", 2e-3, "sigmoid", 0.5, 0.0, 1e-2, None, None, "cross", 0, 12, 80, 4, 11, 271),
    ("a2", "adagrad", 0.1, "softplus", None, 1.0, 0.0, None, None, "normal", 1, 16, 60, 5, 12, 272),
]
OPT_STEPS = 10

PREDICT_CASES = [
    # name, dim, model margin, epsilon, torch_seed
    ("p1", 5, None, None, 281),
    ("p2", 8, None, None, 282),
    ("p3", 20, 30.0, 2.0, 283),
]

# (uniform init within +-2: under xavier at this size the scores of kg_small's candidates are within 1e-6 of each
# other and a quarter of the ranks would be near-ties)
LP_CASE = ("lp", 16, 30.0, 2.0, 298)   # name, dim, model margin, epsilon, torch_seed


def _nan(x):
    return np.nan if x is None else x


def _model(ent, rel, dim, gamma, eps, tseed):
    import torch
    from openke.module.model import DistMult
    torch.manual_seed(tseed)
    return DistMult(ent_tot=ent, rel_tot=rel, dim=dim, margin=gamma, epsilon=eps)


def _build(loss, temp, regul, l3, gamma, eps, sampling, bern, dim, bs, neg, seed, tseed, opt, lr):
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import SigmoidLoss, SoftplusLoss
    from openke.module.strategy import NegativeSampling
    dl = TrainDataLoader(in_path=mg.DATASETS["small"], batch_size=bs, threads=8, sampling_mode=sampling,
                         bern_flag=bern, filter_flag=1, neg_ent=neg, neg_rel=0, random_seed=seed)
    kge = _model(dl.get_ent_tot(), dl.get_rel_tot(), dim, gamma, eps, tseed)
    lo = SigmoidLoss(adv_temperature=temp) if loss == "sigmoid" else SoftplusLoss(adv_temperature=temp)
    ns = NegativeSampling(model=kge, loss=lo, batch_size=dl.get_batch_size(), regul_rate=regul, l3_regul_rate=l3)
    tr = Trainer(model=ns, data_loader=dl, train_times=0, alpha=lr, use_gpu=False, opt_method=opt)
    tr.run()   # builds the optimizer (train_times=0 runs no epoch)
    return dl, kge, tr


def _tables(kge):
    sd = kge.state_dict()
    return {k: sd[k + ".weight"].detach().clone().numpy() for k in TABLES}


def _next_batch(dl, sampling):
    d = dl.cross_sampling() if sampling == "cross" else dl.sampling()
    return {"h": d["batch_h"].copy(), "t": d["batch_t"].copy(), "r": d["batch_r"].copy(), "mode": d["mode"]}, d


def _config(loss, temp, regul, l3, gamma, eps, sampling, dim, bs, neg, seed, tseed, kge):
    rec = dict(model="DistMult", loss=loss, adv_temperature=_nan(temp), regul_rate=regul, l3_regul_rate=l3,
               model_margin=_nan(gamma), epsilon=_nan(eps), sampling=sampling, dim=dim, batch_size=bs, neg_ent=neg,
               seed=seed, torch_seed=tseed, state_keys=np.array(sorted(kge.state_dict().keys())))
    for k, v in _tables(kge).items():
        rec["init_" + k] = v
    return rec


def case_grad(out, name, loss, temp, regul, gamma, eps, sampling, dim, bs, neg, seed, tseed, steps):
    dl, kge, tr = _build(loss, temp, regul, 0.0, gamma, eps, sampling, 0, dim, bs, neg, seed, tseed, "sgd", 1.0)
    rec = _config(loss, temp, regul, 0.0, gamma, eps, sampling, dim, bs, neg, seed, tseed, kge)
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


def case_opt(out, name, opt, lr, loss, temp, regul, l3, gamma, eps, sampling, bern, dim, bs, neg, seed, tseed):
    dl, kge, tr = _build(loss, temp, regul, l3, gamma, eps, sampling, bern, dim, bs, neg, seed, tseed, opt, lr)
    rec = _config(loss, temp, regul, l3, gamma, eps, sampling, dim, bs, neg, seed, tseed, kge)
    losses, modes = [], []
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
    np.savez_compressed(out, optimizer=opt, steps=OPT_STEPS, lr=lr, bern=bern,
                        losses=np.array(losses, dtype=np.float64), modes=np.array(modes), **rec)


def case_predict(out, name, dim, gamma, eps, tseed):
    import torch
    ent, rel, n = 37, 3, 29
    kge = _model(ent, rel, dim, gamma, eps, tseed)
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
    np.savez_compressed(out, model="DistMult", dim=dim, model_margin=_nan(gamma), epsilon=_nan(eps), torch_seed=tseed,
                        state_keys=np.array(sorted(kge.state_dict().keys())), **rec,
                        **{"init_" + k: v for k, v in _tables(kge).items()}, **_tables(kge))


def case_lp(out, name, dim, gamma, eps, tseed):
    from openke.config import Tester
    from openke.data import TestDataLoader
    test_dl = TestDataLoader(mg.DATASETS["small"], "link")
    kge = _model(test_dl.get_ent_tot(), test_dl.get_rel_tot(), dim, gamma, eps, tseed)
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
    np.savez_compressed(out, model="DistMult", dim=dim, model_margin=_nan(gamma), epsilon=_nan(eps), torch_seed=tseed,
                        state_keys=np.array(sorted(kge.state_dict().keys())),
                        metrics=np.array(res, dtype=np.float64), rank_names=np.array(names), ranks=ranks,
                        queries=queries, **{"init_" + k: v for k, v in _tables(kge).items()}, **_tables(kge))


def run_case(kind, args_json, out, tmp):
    args = json.loads(args_json)
    mg._import_reference(tmp)
    mg._silence()
    {"grad": case_grad, "opt": case_opt, "predict": case_predict, "lp": case_lp}[kind](out, *args)


def main():
    subprocess.check_call(["make", "-C", os.path.join(mg.REPO, "oracle"), "ref"])
    tmp = tempfile.mkdtemp(prefix="refpy_")
    jobs = [("grad", list(c), "distmult_%s.npz" % c[0]) for c in GRAD_CASES]
    jobs += [("opt", list(c), "distmult_%s.npz" % c[0]) for c in OPT_CASES]
    jobs += [("predict", list(c), "distmult_%s.npz" % c[0]) for c in PREDICT_CASES]
    jobs += [("lp", list(LP_CASE), "distmult_lp.npz")]
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
