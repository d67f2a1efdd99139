"""The tanh-Gaussian policy head without a GPU: seed_rl_amd/csrc/normal_tanh_math.h (the header the HIP kernel computes
with) built by g++ under AddressSanitizer + UBSan (tests/host/normal_tanh_emul.cpp) and run, element by element and as a
plain-loop version of the whole loss head, against the fp64 oracle (tests/normal_tanh_oracle.py); the Python-side
validation of the Box action space; the additivity the reference's joint-distribution test pins."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import normal_tanh_oracle as nto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
  exe = os.path.join(ROOT, 'build', 'normal_tanh_emul')
  os.makedirs(os.path.dirname(exe), exist_ok=True)
  src = os.path.join(ROOT, 'tests', 'host', 'normal_tanh_emul.cpp')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
                         '-fno-sanitize-recover=all', '-static-libasan', '-Wall', src, '-o', exe])
  tmp = tmp_path_factory.mktemp('nt')

  def run(mode, blobs, out_floats):
    fin, fout = str(tmp / 'in.bin'), str(tmp / 'out.bin')
    with open(fin, 'wb') as f:
      for b in blobs:
        f.write(b if isinstance(b, bytes) else np.ascontiguousarray(b).tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    p = subprocess.run([exe, mode, fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors='replace')[-4000:]       # a sanitizer report ends the test
    out = np.fromfile(fout, np.float32)
    assert out.size == out_floats
    return out
  return run


def test_log_ndtr_is_a_true_log_ndtr(emul):
  z = np.concatenate([np.linspace(-40, 8, 2001), [-20.0, -1.0, -1.0000001, -5.6568542, -5.656855, 0.0]]).astype(np.float32)
  out = emul('ndtr', [struct.pack('<i', z.size), z], 2 * z.size).reshape(-1, 2).astype(np.float64)
  z64 = torch.tensor(z.astype(np.float64), requires_grad=True)
  ref = torch.special.log_ndtr(z64)
  ref.sum().backward()
  ref, dref = ref.detach().numpy(), z64.grad.numpy()
  assert np.all(np.isfinite(out))
  assert abs(out[z == -20.0][0, 0] + 203.917) < 1e-2                          # about -200, not -inf
  # fp32 working precision: a few ulp of the value (the z^2 / 2 term carries the rounding of z itself)
  np.testing.assert_allclose(out[:, 0], ref, rtol=4e-6, atol=1e-7)
  np.testing.assert_allclose(out[:, 1], dref, rtol=4e-6, atol=1e-30)


def _terms64(a, loc, s, eps):
  p = torch.tensor(np.stack([loc, s], -1).astype(np.float64), requires_grad=True)      # D = 1 rows
  lp = nto.log_prob(p, torch.tensor(a)[:, None])
  g_lp, = torch.autograd.grad(lp.sum(), p)
  ent = nto.entropy(p, torch.tensor(eps)[:, None])
  g_en, = torch.autograd.grad(ent.sum(), p)
  return np.stack([lp.detach().numpy(), g_lp[:, 0].numpy(), g_lp[:, 1].numpy(), ent.detach().numpy(),
                   g_en[:, 0].numpy(), g_en[:, 1].numpy()], -1)


def test_per_element_terms_match_fp64_oracle(emul):
  rng = np.random.default_rng(0)
  n = 20000
  loc = rng.uniform(-2, 2, n).astype(np.float32)
  s = rng.uniform(-1, 1, n).astype(np.float32)
  eps = rng.standard_normal(n).astype(np.float32)
  a = np.tanh(rng.standard_normal(n) * 1.5).astype(np.float32)
  special = np.array([1.0, -1.0, 0.999, -0.999, 0.9989999, -0.9989999, 0.0], np.float32)
  a[:7000] = special[rng.integers(0, len(special), 7000)]
  out = emul('terms', [struct.pack('<i', n), a, loc, s, eps], 6 * n).reshape(n, 6).astype(np.float64)
  ref = _terms64(a, loc, s, eps)
  assert np.all(np.isfinite(out)) and np.all(np.isfinite(ref))
  # both clipped ends and the last interior value are present and take different branches
  assert np.all(ref[a == np.float32(0.999), 0] != ref[a == np.float32(0.9989999), 0][0])
  for k, name in enumerate(['log_prob', 'dlp/dloc', 'dlp/ds', 'entropy', 'dH/dloc', 'dH/ds']):
    err = np.abs(out[:, k] - ref[:, k])
    bound = 1e-5 * np.maximum(1.0, np.abs(ref[:, k]))          # fp32 working precision over ~10 roundings
    i = int(np.argmax(err / bound))
    assert err[i] <= bound[i], (name, a[i], loc[i], s[i], out[i, k], ref[i, k])


CFGS = [dict(entropy_cost=0.01, kl_cost=0.0, max_abs_reward=0.0), dict(entropy_cost=0.01, kl_cost=0.1, max_abs_reward=1.0),
        dict(entropy_cost_param=-0.4, entropy_cost_adjustment_speed=10.0, target_entropy=-1.5, kl_cost=0.1,
             max_abs_reward=0.0),
        dict(entropy_cost_param=-0.4, entropy_cost_adjustment_speed=10.0, target_entropy=None, kl_cost=0.0,
             max_abs_reward=1.0)]


def run_host_head(emul, inp, cfg, T, B, mean_denominator=None):
  D, ld = inp['D'], inp['ld']
  has_param = 'entropy_cost_param' in cfg
  n = float(mean_denominator or T * B)
  share = (cfg.get('target_entropy') or 0.0) * (T * B) / n
  ints = struct.pack('<6i', T, B, D, ld, int(has_param), int(bool(cfg.get('target_entropy'))))
  c = np.array([cfg.get('entropy_cost', 0.0), cfg.get('entropy_cost_param', 0.0),
                cfg.get('entropy_cost_adjustment_speed', 0.0), share, 0.5, cfg['kl_cost'], 0.99, 1.0,
                cfg['max_abs_reward'], 1.0, 1.0, n], np.float32)
  N1, N = (T + 1) * B, T * B
  out = emul('loss', [ints, c, inp['head'], inp['beh'], inp['actions'], inp['noise'], inp['rewards'],
                      inp['done'].astype(np.uint8)], N1 * ld + 2 * N + 16 + 1)
  d_head = out[:N1 * ld].reshape(T + 1, B, ld)
  o = N1 * ld
  return dict(d_head=d_head, d_params=d_head[..., :2 * D], d_baseline=d_head[..., 2 * D], vs=out[o:o + N].reshape(T, B),
              pg=out[o + N:o + 2 * N].reshape(T, B), scalars=out[o + 2 * N:o + 2 * N + 13],
              d_entropy_cost_param=float(out[-1]) if has_param else None)


@pytest.mark.parametrize('cfg', range(len(CFGS)))
@pytest.mark.parametrize('B,D', [(3, 1), (3, 17), (32, 6), (32, 64), (7, 64)])
def test_host_head_matches_fp64_oracle(emul, B, D, cfg):
  """The plain-loop head on the header's maths, under the sanitizers, held to the gate the GPU kernel is held to; also
  checks that the fp32 oracle itself is finite on these inputs (the gate is meaningless otherwise)."""
  T, cfg = 20, CFGS[cfg]
  inp = nto.make_inputs(100 * B + D, T, B, D)
  got = run_host_head(emul, inp, cfg, T, B)
  r32, r64 = nto.evaluate(inp, torch.float32, **cfg), nto.evaluate(inp, torch.float64, **cfg)
  for r in (r32, r64):
    assert all(np.all(np.isfinite(r[k])) for k in ('scalars', 'vs', 'pg', 'd_params', 'd_baseline'))
  res = nto.gate(got, r32, r64)
  print('B=%d D=%d %s' % (B, D, {k: '%.3g/%.3g (x%.2f)' % v for k, v in res.items()}))
  for k, (dist, allowed, _) in res.items():
    assert dist <= allowed, (k, dist, allowed)
  if got['d_entropy_cost_param'] is not None:
    assert abs(got['d_entropy_cost_param'] - r64['d_entropy_cost_param']) <= \
        2 * abs(r32['d_entropy_cost_param'] - r64['d_entropy_cost_param']) + 2e-5 * max(1.0, abs(r64['d_entropy_cost_param']))
  # containment: pad columns keep the 7.0 they were filled with, everything in range was overwritten, bootstrap row zero
  assert np.all(got['d_head'][..., 2 * D + 1:] == 7.0)
  assert not np.any(got['d_head'][..., :2 * D + 1] == 7.0)
  assert np.all(got['d_head'][-1, :, :2 * D + 1] == 0.0)


def test_host_head_replica_shares(emul):
  T, B, D = 20, 8, 6
  cfg = CFGS[2]
  inp = nto.make_inputs(3, T, B, D)
  full = run_host_head(emul, inp, cfg, T, B)
  parts = []
  for sl in (slice(0, 4), slice(4, 8)):
    sub = dict((k, np.ascontiguousarray(v[:, sl]) if isinstance(v, np.ndarray) else v) for k, v in inp.items())
    parts.append(run_host_head(emul, sub, cfg, T, 4, mean_denominator=T * B))
  assert abs(parts[0]['scalars'][0] + parts[1]['scalars'][0] - full['scalars'][0]) < 1e-5 * max(1.0, abs(full['scalars'][0]))
  np.testing.assert_allclose(np.concatenate([p['d_params'] for p in parts], 1), full['d_params'], rtol=1e-5, atol=1e-8)


def test_additivity_with_the_joint_test_numbers():
  """common/parametric_distribution_test.py:50-84 of the reference: locs 0, scale parameters .1 / .2 / .3, actions 0 and
  .99 -- the log_prob of the 3-vector is the sum of the three 1-D log_probs, and finite."""
  for act in (0.0, 0.99):
    p3 = torch.tensor([0., 0., 0., .1, .2, .3], dtype=torch.float64)
    whole = nto.log_prob(p3, torch.full((3,), act, dtype=torch.float64))
    parts = sum(nto.log_prob(torch.tensor([0., sc], dtype=torch.float64), torch.tensor([act], dtype=torch.float64))
                for sc in (.1, .2, .3))
    assert np.isfinite(float(whole)) and abs(float(whole) - float(parts)) < 1e-12


def test_box_space_gives_the_tanh_gaussian():
  """Fails on a tree without the feature: a Box space used to raise NotImplementedError."""
  from seed_rl_amd import parametric_distribution as pd
  for D in (1, 6, 17):
    dist = pd.get_parametric_distribution_for_action_space(pd.Box(-1.0, 1.0, shape=(D,)))
    assert dist.param_size == 2 * D and dist.num_actions == D and dist.reparametrizable
    assert dist.loss_head == 'normal_tanh'
  assert pd.normal_tanh_distribution(4).param_size == 8
  cat = pd.get_parametric_distribution_for_action_space(pd.Discrete(5))
  assert cat.param_size == 5 and cat.loss_head == 'categorical' and not cat.reparametrizable


def test_box_space_validation():
  from seed_rl_amd import parametric_distribution as pd
  with pytest.raises(ValueError, match=r'bounded to \[-1,1\]'):
    pd.get_parametric_distribution_for_action_space(pd.Box(-2.0, 1.0, shape=(3,)))
  with pytest.raises(ValueError, match=r'bounded to \[-1,1\]'):
    pd.get_parametric_distribution_for_action_space(pd.Box(np.array([-1., -1.]), np.array([1., 0.5])))
  with pytest.raises(AssertionError):
    pd.get_parametric_distribution_for_action_space(pd.Box(-1.0, 1.0, shape=(2, 2)))
  with pytest.raises(ValueError):
    pd.normal_tanh_distribution(65)

  class MultiDiscrete(object):
    nvec = [3, 3]
  for space in (MultiDiscrete(), (pd.Discrete(2), pd.Box(-1.0, 1.0, shape=(1,)))):
    with pytest.raises(NotImplementedError, match='MultiDiscrete.*Tuple.*ClippedIdentity.*shifted std'):
      pd.get_parametric_distribution_for_action_space(space)
  with pytest.raises(NotImplementedError, match='ClippedIdentity'):
    pd.get_parametric_distribution_for_action_space(pd.Box(-1.0, 1.0, shape=(2,)), continuous_config=object())


def test_entry_points_validate_before_launching():
  """Argument validation happens before any launch, so it runs without a GPU (as tests/test_abi.py does)."""
  from seed_rl_amd import build, _lib
  build.build()
  l = _lib.lib()
  one = (_lib.c_float * 64)()
  p = _lib.ctypes.cast(one, _lib.c_void_p)

  def loss(T=2, B=2, D=2, ld=8, ws=4096, params=p, ecp=None, decp=None, has_target=0, noise=p, n=4.0):
    return l.seedhip_normal_tanh_loss_fwd_bwd(params, ld, p, ld, p, p, noise, p, p, T, B, D, 0.01, ecp, 10.0, has_target,
                                              0.0, decp, 0.5, 0.0, 0.99, 1.0, 0.0, 1.0, 1.0, n, p, p, None, None, p, p,
                                              ws, None)
  for kw, msg in ((dict(D=0), b'outside 1..64'), (dict(D=65, ld=200), b'outside 1..64'), (dict(ld=3), b'row strides'),
                  (dict(params=None), b'null pointer'), (dict(noise=None), b'null pointer'), (dict(ws=4), b'workspace'),
                  (dict(T=0), b'T>=1'), (dict(ecp=p), b'go together'), (dict(has_target=1), b'learnable'),
                  (dict(T=20000), b'too long for LDS'), (dict(n=0.0), b'mean_denominator')):
    if 'T' in kw and kw['T'] > 100:
      kw['ws'] = 1 << 20
    assert loss(**kw) == -1 and msg in l.seedhip_last_error(), (kw, l.seedhip_last_error())
  lpe = l.seedhip_normal_tanh_log_prob_entropy
  assert lpe(None, None, None, 0, 3, None, None, None) == 0                   # rows == 0: nothing to do
  assert lpe(None, None, None, -1, 3, None, None, None) == -1
  assert lpe(p, None, None, 4, 3, p, None, None) == -1 and b'needs actions' in l.seedhip_last_error()
  assert lpe(p, None, None, 4, 3, None, p, None) == -1 and b'noise' in l.seedhip_last_error()
  assert lpe(p, p, p, 4, 65, p, p, None) == -1
  smp = l.seedhip_normal_tanh_sample
  assert smp(p, 5, 4, 3, p, p, None) == -1 and b'ld' in l.seedhip_last_error()  # ld < 2 D
  assert smp(p, 6, 4, 3, None, p, None) == -1 and b'rng_state' in l.seedhip_last_error()
  assert smp(p, 6, -1, 3, p, p, None) == -1
  assert l.seedhip_normal_fill(p, -1, p, None) == -1
  assert l.seedhip_normal_fill(p, 8, None, None) == -1
