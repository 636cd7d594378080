"""Generate the golden vector of the wide-dim tests (tests/golden/wide_g1.npz).

Needs the reference tree and oracle/_ref/Base.so:

    python tests/golden/make_golden_wide.py

Same recipe as make_golden_adv.py (whose helpers it uses): the reference's own Trainer.train_one_step on kg_small, on
CPU, in a subprocess. One case: TransE at dim 1024 in the configuration of examples/train_transe_WN18_adv_sigmoidloss.py
(p_norm 1, no normalisation, margin 6, epsilon 2, SigmoidLoss(adv_temperature=1)), one step of SGD at lr 1 on a batch of
11 positives with 3 negatives each, so the table delta is the reference's float32 gradient. Only the rows the batch
touches are recorded (a whole entity table is 3 MB at this dim); the script checks that no other row moved.
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
import make_golden_adv as mga  # noqa: E402

# name, loss, adv_temperature, loss margin, p_norm, norm_flag, model margin, epsilon, sampling, dim, bs, neg, seed,
# torch_seed
CASE = ("g1", "sigmoid", 1.0, None, 1, False, 6.0, 2.0, "normal", 1024, 11, 3, 21, 61)


def case_wide(out, name, loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed):
    dl, kge, tr = mga._build("TransE", loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed,
                             "sgd", 1.0)
    rec = mga._config("TransE", loss, temp, lmargin, p, nf, gamma, eps, sampling, dim, bs, neg, seed, tseed)
    before = mga._tables(kge)
    b, d = mga._next_batch(dl, sampling)
    step_loss = tr.train_one_step(d)
    after = mga._tables(kge)
    rows = {"ent_embeddings": np.unique(np.concatenate([b["h"], b["t"]])), "rel_embeddings": np.unique(b["r"])}
    for k, ids in rows.items():
        moved = np.nonzero((before[k] != after[k]).any(axis=1))[0]
        assert np.isin(moved, ids).all(), k
        rec["rows_" + k] = ids.astype(np.int64)
        rec["s0_" + k] = before[k][ids]
        rec["s1_" + k] = after[k][ids]
    np.savez_compressed(out, lr=1.0, losses=np.array([step_loss], dtype=np.float64), mode=b["mode"], b_h=b["h"],
                        b_t=b["t"], b_r=b["r"], **rec)


def main():
    subprocess.check_call(["make", "-C", os.path.join(mg.REPO, "oracle"), "ref"])
    tmp = tempfile.mkdtemp(prefix="refpy_")
    print("generating wide_g1.npz", flush=True)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", json.dumps(list(CASE)),
                           os.path.join(HERE, "wide_g1.npz"), tmp])
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        mg._import_reference(sys.argv[4])
        mg._silence()
        case_wide(sys.argv[3], *json.loads(sys.argv[2]))
    else:
        main()
