"""bench.py's two kinds of run (-m gpu): a plain run does only what its headline figure needs (no kernel-section pass, no CPU baseline), and
--full adds both after the timed steps without touching them: on the same seeded configuration the two deliver the same bytes, unit by unit."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, name, extra):
    env = dict(os.environ, AGX_BENCH_DIGEST=str(tmp_path / (name + ".json")))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "custom",
                        "--chroms", "400000,250000", "--pairs", "60000", "--workdir", str(tmp_path / name)] + extra,
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return line, json.load(open(tmp_path / (name + ".json")))


def test_full_adds_its_legs_and_leaves_the_timed_steps_alone(tmp_path):
    plain, plain_out = _bench(tmp_path, "plain", [])
    assert plain["full"] is False and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["cpu_baseline"] is None and plain["breakdown_ms_largest_unit"] is None and "graph_largest_unit" not in plain
    full, full_out = _bench(tmp_path, "full", ["--full", "--cpu-sample-pairs", "2000"])
    assert full["full"] is True
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["parallel"]["value"] > 0
    assert full["breakdown_ms_largest_unit"]["ms_node_sweep"] > 0
    assert full["graph_largest_unit"]["positions"] == full["units"]["0"]["positions"]
    assert sorted(plain_out) == ["0", "1"]
    assert plain_out == full_out, "a --full run delivered other bytes than a plain run"
