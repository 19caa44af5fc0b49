"""bench.py end to end on the MI355X, as a fresh child process: a plain run times exactly --steps steps, prints the ONE line with
its headline fields and nothing of what --full adds, and --dump-outputs writes the last step's tables and loss."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SMALL = ['--users', '20000', '--items', '4000', '--nnz', '1000000', '--rank', '32', '--samples', '64']


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / 'outputs'
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(out)] + SMALL
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['metric'] == 'train_interactions_per_sec' and line['unit'] == 'interactions/s' and line['higher_is_better'] is True
    assert line['dtype'] == 'f32' and line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(line['config']['interactions_total'] / (line['ms_per_step'] * 1e-3), rel=1e-4)
    assert not {'cpu_baseline', 'predict_rows_per_sec', 'recall_at_10', 'hbm_legs', 'extras'} & set(line)   # --full only
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {'user_factors', 'user_rows', 'item_factors', 'item_rows', 'loss'}
    assert got['user_factors'].shape == (20000, 32) and got['item_factors'].shape == (4000, 32)        # small tables: whole
    assert np.array_equal(got['user_rows'], np.arange(20000.0)) and np.array_equal(got['item_rows'], np.arange(4000.0))
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert got['loss'].shape == (1,) and got['loss'][0] > 0
    assert not np.all(got['user_factors'] == 0) and not np.all(got['item_factors'] == 0)
