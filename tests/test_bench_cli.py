"""bench.py's two depths: a plain run prints the headline line and measures nothing else; everything that takes runs of its own sits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ONLY_FULL = ("quality", "end_to_end", "end_to_end_metric", "strong_scaling", "two_batches_in_flight", "secondary", "cpu_baseline")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


def test_full_is_an_option_and_off_by_default():
    """--full parses (here on the CPU rehearsal path, which measures nothing either way) and is documented; an unknown option still is an error."""
    p = subprocess.run([sys.executable, BENCH, "--mock", "--full", "--glyphs", "512"], capture_output=True, text=True, timeout=300, env=_env())
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])["glyphs_per_rank"] == [512]
    h = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120, env=_env())
    assert h.returncode == 0 and "--full" in h.stdout
    bad = subprocess.run([sys.executable, BENCH, "--mock", "--fuller"], capture_output=True, text=True, timeout=120, env=_env())
    assert bad.returncode != 0


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_nothing_that_moved(tmp_path):
    """A plain run: ONE JSON line on stdout with the contract fields, consistent among themselves, the dump of the last step's tiles, and none of the
    entries that take runs of their own."""
    g, steps = 512, 2
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--glyphs", str(g), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, env=_env(), cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "MSDF glyphs/sec (64x64, fp32)" and d["unit"] == "glyphs/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and abs(d["value"]-g/(d["ms_per_step"]*1e-3)) <= 1e-9*d["value"]
    assert not [k for k in ONLY_FULL if k in d], sorted(d)
    tiles, index = np.load(tmp_path/"tiles.npy"), np.load(tmp_path/"tiles_index.npy")
    assert tiles.shape == (g, 64, 64, 3) and tiles.dtype == np.float32 and index.tolist() == list(range(g))
    assert np.load(tmp_path/"tiles_nonfinite.npy").shape == (g, 3)
