"""bench.py --dump-outputs: what the last timed step computed, as float32 / float64 .npy files of at most 64 MB,
the same from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(out_dir):
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_samples_and_caps_what_does_not_fit(tmp_path):
    import torch

    import bench

    rng = np.random.default_rng(1)
    res, merged, units = [], {}, [5, 2, 9]
    for u, n in zip(units, [700000, 300000, 400000]):
        res.append({"n": n, "scores": torch.from_numpy(rng.random(n)),
                    "solution": torch.from_numpy((rng.random(n) < 0.1).astype(np.uint8)),
                    "selection_penalty": rng.random(), "selected_count": 7, "penalized_objective": 1.5})
        merged[u] = rng.integers(0, n, (3000000 if u == 9 else 1000, 2))  # more rows than 64 MB hold
    bench.dump_outputs(str(tmp_path), res, merged, units)
    got = _load(tmp_path)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["chromosome_index"].tolist() == [2.0, 5.0, 9.0]
    pos = got["sample_locus"].astype(np.int64)
    by_unit = [res[1], res[0], res[2]]
    assert np.array_equal(np.concatenate([r["scores"].numpy() for r in by_unit])[pos], got["scores_sample"])
    assert np.array_equal(np.concatenate([r["solution"].numpy() for r in by_unit])[pos], got["solution_sample"])
    rows = np.concatenate([np.column_stack([np.full(len(merged[u]), u), merged[u]]) for u in sorted(merged)])
    assert np.array_equal(rows[got["interval_row"].astype(np.int64)], got["intervals"])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_dump_is_the_same_from_run_to_run(gpu, tmp_path):
    outs = []
    for run, steps in (("a", 2), ("b", 1)):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--chroms", "chr21,chr22", "--steps", str(steps),
               "--warmup", "1", "--dump-outputs", str(tmp_path / run)]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        assert proc.returncode == 0, proc.stderr[-2000:]
        line = json.loads([t for t in proc.stdout.splitlines() if t.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        outs.append(_load(tmp_path / run))
    a, b = outs
    assert sorted(a) == sorted(b) and "interval_row" not in a
    for name in a:
        assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), name
    assert a["chromosome_index"].tolist() == [0.0, 1.0]  # positions in the --chroms list
    assert a["intervals"].shape[1] == 3 and np.all(a["intervals"][:, 1] < a["intervals"][:, 2])
    assert 0 < (a["intervals"][:, 2] - a["intervals"][:, 1]).sum() <= a["selected_count"].sum()
