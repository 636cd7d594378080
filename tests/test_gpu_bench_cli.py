"""bench.py's plain run from the command line: --steps timed steps, the headline line only, and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "pu_c3", "pu_c3_ref6000", "cpu_baseline", "deterministic_ms_per_step", "ms_per_step_runs")


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_outputs(tmp_path):
    steps = 3
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--data-dir", str(tmp_path / "data"), "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    for k in HEADLINE:
        assert k in rec, k
    for k in FULL_ONLY:   # measured only with --full
        assert k not in rec, k
    assert rec["steps"] == steps and rec["unit"] == "triples/s" and rec["higher_is_better"] is True
    slots = rec["config"]["slots_per_step_per_gpu"]
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(slots * 1e3 / rec["ms_per_step"], rel=1e-9)
    got = {f: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["ent_embeddings.npy", "losses.npy", "rel_embeddings.npy"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["losses.npy"].shape == (steps,)   # one loss per timed step: --steps sets their number
    assert float(got["losses.npy"][-1]) == pytest.approx(rec["loss_last_step"], rel=1e-6)
    assert got["ent_embeddings.npy"].ndim == 2 and got["ent_embeddings.npy"].shape[1] == 200
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
