"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run (no --full) -- the headline line alone, exactly K timed steps, and
`--dump-outputs DIR`: the last timed step's loss and the parameters after it as float .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    out = tmp_path / 'outputs'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '24', '--warmup', '2', '--dump-outputs', str(out),
           '--watchdog', '300']
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=400)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{'), 'the result line must be the ONLY line on stdout'
    line = json.loads(lines[0])
    assert line['steps'] == 24 and line['warmup'] == 2 and line['n_gpus'] == 1 and line['full'] is False
    assert line['unit'] == 'samples/s' and line['higher_is_better'] is True and line['dtype'] == 'f16'
    assert line['ms_per_step'] > 0 and line['value'] > 0
    assert line['config']['captures_in_timed_region'] == 0 and 'hip-graph replay' in line['config']['execution']
    # a plain run measures the headline only
    for key in ('roofline', 'rooflines', 'cpu_baseline', 'dropin_path', 'render_800x800_ms', 'strong_scaling', 'sdf_encoder_mlp', 'tnt_bound8',
                'evolving_occupancy', 'ddp_overhead_1rank'):
        assert not line[key], key
    files = sorted(os.listdir(out))
    assert 'loss.npy' in files and 'param_encoder_embeddings.npy' in files, files
    total = 0
    for f in files:
        a = np.load(out / f)
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(out / 'loss.npy')[0]) == line['config']['final_loss']
