"""The 8-wave instances of the plane predict kernels (tmf_predict_split.hip): the dispatcher picks them only under TMF_SPLIT_WAVES=8
(A/B runs), which the library reads once per process - so they run in a fresh child process (tests/split_8waves_child.py)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_eight_wave_plane_kernels_in_a_child_process():
    env = {**os.environ, 'TMF_SPLIT_WAVES': '8'}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'split_8waves_child.py')], env=env, capture_output=True, text=True,
                       timeout=900)
    print(p.stdout[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert '8-wave plane kernels: 64 cases ok' in p.stdout
