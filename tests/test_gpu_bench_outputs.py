"""A plain `bench.py` run does only what its headline figure needs, --steps sets its timed steps, and --dump-outputs
writes what the last timed step computed.  A `--full` run of the same arguments adds the attribution pass, the extra
windows and the other records around the SAME timed path: its dump must be identical, element for element."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, STEPS = 32, 20, 4


def _bench(*args):
  env = dict(os.environ)
  env.pop('RANK', None); env.pop('WORLD_SIZE', None); env.pop('LOCAL_RANK', None)
  cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', '2',
         '--batch', str(B)] + list(args)
  r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                     universal_newlines=True)
  assert r.returncode == 0, r.stderr[-3000:]
  lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{') and '"metric"' in l]
  assert len(lines) == 1, r.stdout[-2000:]
  return lines[0]


def _load(d):
  return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')}


def test_plain_run_dumps_what_the_full_run_computes(device, tmp_path):
  plain = _bench('--dump-outputs', str(tmp_path / 'plain'))
  assert plain['unit'] == 'env-frames/s' and plain['higher_is_better'] is True and plain['dtype'] == 'f32'
  assert plain['steps'] == STEPS and plain['ms_per_step'] > 0
  assert plain['value'] == pytest.approx(B * T / (plain['ms_per_step'] * 1e-3), rel=1e-3)
  assert not set(plain) & {'roofline', 'windows', 'step_roofline', 'kernels_ms_per_step', 'vtrace_max_abs_err',
                           'parity', 'cpu_baseline', 'tail_summary'}
  full = _bench('--full', '--quick', '--dump-outputs', str(tmp_path / 'full'))
  assert full['roofline']['kernel'] and full['windows']['count'] == 6 and 'vtrace_max_abs_err' in full
  a, b = _load(tmp_path / 'plain'), _load(tmp_path / 'full')
  assert {'loss', 'log_losses_total', 'params', 'grads'} <= set(a) and set(a) == set(b)
  assert sum(x.nbytes for x in a.values()) <= 64e6
  for k in a:
    assert a[k].dtype in (np.float32, np.float64), k
    assert np.all(np.isfinite(a[k])), k
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)
  assert float(a['loss']) == pytest.approx(plain['loss'], abs=1e-6)
  assert a['params'].size >= plain['config']['params']              # the flat buffer (tensors padded to 4 floats)
