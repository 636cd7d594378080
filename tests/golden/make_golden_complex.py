"""Generate the golden vectors of ComplEx (tests/golden/complex_*.npz).

Needs the reference tree and oracle/_ref/Base.so:

    python tests/golden/make_golden_complex.py

Same recipe as make_golden_distmult.py (whose helpers it uses through make_golden.py): the reference's Python package is
imported from a throw-away copy with oracle/_ref/Base.so, on CPU, one subprocess per case. The fixtures hold data
only (configs, batches, tables, losses, optimizer state, scores, ranks).

  complex_g*.npz  gradient cases: the reference's Trainer.train_one_step under SGD at lr 1 for 2-3 steps, the four
                  tables recorded before and after every step, so each step's table delta is the reference's float32
                  gradient at the tables before it. SigmoidLoss and SoftplusLoss, each with and without the
                  adversarial weights, regul_rate 0 and 1, normal sampling (g4 with neg_rel = 2), dims 5, 7, 8, 12, 16, 20.
  complex_a*.npz  one Adagrad trajectory with regul_rate 1 and bern_flag 1 (examples/train_complex_WN18.py in
                  miniature) and one Adam trajectory, 10 steps each: losses, batches, initial and final tables, the
                  optimizer state after step 1 and at the end.
  complex_p*.npz  the reference's predict (-score) in the three modes on recorded tables.
  complex_lp.npz  the reference Tester's metrics and per-query raw / filtered ranks on kg_small. Under xavier at
                  kg_small's size the candidates' scores nearly tie and ComplEx has no uniform init branch, so the
                  four tables are overwritten with seeded uniform(+-2) draws before testing, and recorded.
Every file records state_keys (the model's state_dict keys) and the four init_* tables of its seeded construction.

Cross sampling: ComplEx.forward ignores data['mode'] (ComplEx.py:29-40), so a cross-sampled batch ([B (1 + K)] on the
varying side, [B] on the others, TrainDataLoader.py:199-241) does not broadcast; `--check-cross` runs one such step on
the CPU and reports the error the reference raises.
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

TABLES = ("ent_re_embeddings", "ent_im_embeddings", "rel_re_embeddings", "rel_im_embeddings")

GRAD_CASES = [
    # name, loss, adv_temperature, regul_rate, neg_rel, dim, bs, neg, seed, torch_seed, steps
    ("g1", "sigmoid", 0.5, 0.0, 0, 8, 50, 4, 3, 361, 2),
    ("g2", "softplus", None, 1.0, 0, 5, 40, 6, 4, 362, 3),
    ("g3", "softplus", 1.0, 1.0, 0, 12, 60, 3, 5, 363, 2),
    ("g4", "sigmoid", None, 0.0, 2, 7, 30, 5, 6, 364, 2),
    ("g5", "sigmoid", 1.0, 1.0, 0, 20, 50, 5, 7, 365, 2),
    ("g6", "softplus", None, 0.0, 0, 16, 33, 4, 8, 366, 3),
]

OPT_CASES = [
    # name, optimizer, lr, loss, adv_temperature, regul_rate, bern, dim, bs, neg, seed, torch_seed
    ("a1", "adagrad", 0.5, "softplus", None, 1.0, 1, 20, 60, 5, 11, 371),
    ("a2", "adam", 2e-3, "sigmoid", 0.5, 0.0, 0, 12, 80, 4, 12, 372),
]
OPT_STEPS = 10

PREDICT_CASES = [("p1", 5, 381), ("p2", 8, 382), ("p3", 20, 383)]   # name, dim, torch_seed
LP_CASE = ("lp", 16, 398)   # name, dim, torch_seed
LP_RANGE = 2.0


def _nan(x):
    return np.nan if x is None else x


def _model(ent, rel, dim, tseed):
    import torch
    from openke.module.model import ComplEx
    torch.manual_seed(tseed)
    return ComplEx(ent_tot=ent, rel_tot=rel, dim=dim)


def _build(loss, temp, regul, sampling, bern, neg_rel, dim, bs, neg, seed, tseed, opt, lr):
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import SigmoidLoss, SoftplusLoss
    from openke.module.strategy import NegativeSampling
    dl = TrainDataLoader(in_path=mg.DATASETS["small"], batch_size=bs, threads=8, sampling_mode=sampling,
                         bern_flag=bern, filter_flag=1, neg_ent=neg, neg_rel=neg_rel, random_seed=seed)
    kge = _model(dl.get_ent_tot(), dl.get_rel_tot(), dim, tseed)
    lo = SigmoidLoss(adv_temperature=temp) if loss == "sigmoid" else SoftplusLoss(adv_temperature=temp)
    ns = NegativeSampling(model=kge, loss=lo, batch_size=dl.get_batch_size(), regul_rate=regul)
    tr = Trainer(model=ns, data_loader=dl, train_times=0, alpha=lr, use_gpu=False, opt_method=opt)
    tr.run()   # builds the optimizer (train_times=0 runs no epoch)
    return dl, kge, tr


def _tables(kge):
    sd = kge.state_dict()
    return {k: sd[k + ".weight"].detach().clone().numpy() for k in TABLES}


def _next_batch(dl):
    d = dl.sampling()
    return {"h": d["batch_h"].copy(), "t": d["batch_t"].copy(), "r": d["batch_r"].copy(), "mode": d["mode"]}, d


def _config(loss, temp, regul, neg_rel, dim, bs, neg, seed, tseed, kge):
    rec = dict(model="ComplEx", loss=loss, adv_temperature=_nan(temp), regul_rate=regul, sampling="normal",
               neg_rel=neg_rel, dim=dim, batch_size=bs, neg_ent=neg, seed=seed, torch_seed=tseed,
               state_keys=np.array(sorted(kge.state_dict().keys())))
    for k, v in _tables(kge).items():
        rec["init_" + k] = v
    return rec


def case_grad(out, name, loss, temp, regul, neg_rel, dim, bs, neg, seed, tseed, steps):
    dl, kge, tr = _build(loss, temp, regul, "normal", 0, neg_rel, dim, bs, neg, seed, tseed, "sgd", 1.0)
    rec = _config(loss, temp, regul, neg_rel, dim, bs, neg, seed, tseed, kge)
    losses, modes = [], []
    for k, v in _tables(kge).items():
        rec["s0_" + k] = v
    for s in range(steps):
        b, d = _next_batch(dl)
        for k in ("h", "t", "r"):
            rec["b%d_%s" % (s, k)] = b[k]
        modes.append(b["mode"])
        losses.append(tr.train_one_step(d))
        for k, v in _tables(kge).items():
            rec["s%d_%s" % (s + 1, k)] = v
    np.savez_compressed(out, steps=steps, lr=1.0, losses=np.array(losses, dtype=np.float64), modes=np.array(modes),
                        **rec)


def case_opt(out, name, opt, lr, loss, temp, regul, bern, dim, bs, neg, seed, tseed):
    dl, kge, tr = _build(loss, temp, regul, "normal", bern, 0, dim, bs, neg, seed, tseed, opt, lr)
    rec = _config(loss, temp, regul, 0, dim, bs, neg, seed, tseed, kge)
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
        b, d = _next_batch(dl)
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


def case_predict(out, name, dim, tseed):
    import torch
    ent, rel, n = 37, 3, 29
    kge = _model(ent, rel, dim, tseed)
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
    np.savez_compressed(out, model="ComplEx", dim=dim, torch_seed=tseed,
                        state_keys=np.array(sorted(kge.state_dict().keys())), **rec,
                        **{"init_" + k: v for k, v in _tables(kge).items()}, **_tables(kge))


def case_lp(out, name, dim, tseed):
    import torch
    from openke.config import Tester
    from openke.data import TestDataLoader
    test_dl = TestDataLoader(mg.DATASETS["small"], "link")
    kge = _model(test_dl.get_ent_tot(), test_dl.get_rel_tot(), dim, tseed)
    init = {"init_" + k: v for k, v in _tables(kge).items()}
    rng = np.random.default_rng(tseed)
    for k in TABLES:   # (see the module docstring)
        w = getattr(kge, k).weight.data
        w.copy_(torch.from_numpy(rng.uniform(-LP_RANGE, LP_RANGE, size=tuple(w.shape)).astype(np.float32)))
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
    np.savez_compressed(out, model="ComplEx", dim=dim, torch_seed=tseed, table_range=LP_RANGE,
                        state_keys=np.array(sorted(kge.state_dict().keys())),
                        metrics=np.array(res, dtype=np.float64), rank_names=np.array(names), ranks=ranks,
                        queries=queries, **init, **_tables(kge))


def case_cross(out):
    """One cross-sampled step of the reference on the CPU: prints the error it raises (nothing is written)."""
    dl, kge, tr = _build("softplus", None, 0.0, "cross", 0, 0, 8, 50, 4, 3, 361, "sgd", 1.0)
    try:
        tr.train_one_step(dl.cross_sampling())
    except Exception as e:   # noqa: BLE001  (whatever it raises is the finding)
        print("cross sampling raises %s: %s" % (type(e).__name__, e), file=sys.stderr)   # (stdout is silenced)
        return
    print("cross sampling trained a step", file=sys.stderr)


def run_case(kind, args_json, out, tmp):
    args = json.loads(args_json)
    mg._import_reference(tmp)
    mg._silence()
    if kind == "cross":
        return case_cross(out)
    {"grad": case_grad, "opt": case_opt, "predict": case_predict, "lp": case_lp}[kind](out, *args)


def main():
    subprocess.check_call(["make", "-C", os.path.join(mg.REPO, "oracle"), "ref"])
    tmp = tempfile.mkdtemp(prefix="refpy_")
    if sys.argv[1:] == ["--check-cross"]:
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", "cross", "[]", "-", tmp])
        shutil.rmtree(tmp, ignore_errors=True)
        return
    jobs = [("grad", list(c), "complex_%s.npz" % c[0]) for c in GRAD_CASES]
    jobs += [("opt", list(c), "complex_%s.npz" % c[0]) for c in OPT_CASES]
    jobs += [("predict", list(c), "complex_%s.npz" % c[0]) for c in PREDICT_CASES]
    jobs += [("lp", list(LP_CASE), "complex_lp.npz")]
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
