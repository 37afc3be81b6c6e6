"""bench.py --dump-outputs: what the headline's last timed step computed, as float32 .npy files within 64 MB; the engine
takes exactly 1 + --warmup + --steps steps, so the files depend on warmup + steps and on nothing else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import REPO  # noqa: E402


def _bench(out_dir, steps, warmup, *flags):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--no-alts", "--no-cpu-baseline", "--dump-outputs", str(out_dir), *flags]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == steps and out["warmup"] == warmup and out["timing"]["repeats"] == 1
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return out, arrays


def test_dump_outputs_are_the_last_step_and_set_by_the_step_count(tmp_path):
    from rawaudiovae_kelsey_amd.engine import PARAM_NAMES
    out_a, a = _bench(tmp_path / "a", 3, 1, "--step-kernels-only")
    # the same batches in the same order (1 + 2 + 2 = 1 + 1 + 3 steps), on the default path and with --full: settle_clocks'
    # scratch engine and the per-launch timing (after the dump) leave the headline's outputs alone
    out_b, b = _bench(tmp_path / "b", 2, 2)
    out_f, f = _bench(tmp_path / "f", 2, 2, "--full")
    assert out_b["roofline"] is None and "kernels" not in out_b          # a plain run times the headline alone
    assert len(out_f["kernels"]) == 9 and out_f["roofline"]["us_per_launch"] > 0
    _, c = _bench(tmp_path / "c", 4, 1, "--step-kernels-only")       # one step more
    names = {"loss", "mu", "logvar"} | set(PARAM_NAMES) | {p + k for p in ("exp_avg.", "exp_avg_sq.") for k in PARAM_NAMES}
    assert set(a) == names
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["fc1.weight"].shape == (2048, 1024) and a["mu"].shape == (4096, 64) and a["loss"].shape == (3,)
    assert a["loss"][0] == np.float32(out_a["final_loss"])
    assert all(np.isfinite(v).all() for v in a.values())
    for k in names:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], f[k]), k
    assert not np.array_equal(a["fc1.weight"], c["fc1.weight"]) and a["loss"][0] != c["loss"][0]
