"""Continuous actions on the GPU: the fused V-trace loss head of the tanh-Gaussian policy (csrc/loss_normal_tanh.hip)
against the torch-CPU oracle (tests/normal_tanh_oracle.py; parity with TensorFlow Probability itself is unpinned, see
there), containment of every output buffer, replica shares, the sampler, and a learner step of MLPandLSTM built on the
distribution -- eager and replayed from a HIP graph."""
import itertools

import numpy as np
import pytest
import torch

from oracle import nets_torch
from tests import normal_tanh_oracle as nto

pytestmark = pytest.mark.gpu

GUARD, POISON, FILL = 64, -1234.5, 7.0


def _guarded(device, n):
  """n floats filled with 7.0 between two runs of 64 poisoned floats."""
  big = torch.full((n + 2 * GUARD,), FILL, dtype=torch.float32, device=device)
  big[:GUARD] = POISON
  big[GUARD + n:] = POISON
  return big, big[GUARD:GUARD + n]


def _intact(big):
  b = big.cpu().numpy()
  return bool(np.all(b[:GUARD] == POISON) and np.all(b[-GUARD:] == POISON))


def _to(device, a):
  return torch.as_tensor(np.ascontiguousarray(a)).to(device)


def _kernel(device, inp, cfg, T, B, mean_denominator=None):
  """Runs the head on make_inputs(); every output lives between poisoned guards.  Returns the gate's dict + d_head."""
  from seed_rl_amd import ops
  D, ld = inp['D'], inp['ld']
  N1, N = (T + 1) * B, T * B
  head = _to(device, inp['head']).view(-1)
  bufs = dict(d_head=_guarded(device, N1 * ld), vs=_guarded(device, N), pg=_guarded(device, N),
              scalars=_guarded(device, 16), d_ecp=_guarded(device, 1))
  ws_big, ws = _guarded(device, ops.impala_loss_workspace_bytes(T, B) // 4)
  kw = dict(baseline_cost=0.5, kl_cost=cfg['kl_cost'], discounting=0.99, lambda_=1.0, max_abs_reward=cfg['max_abs_reward'],
            mean_denominator=mean_denominator)
  if 'entropy_cost_param' in cfg:
    share = cfg['target_entropy'] * (T * B) / float(mean_denominator or T * B) if cfg['target_entropy'] else None
    kw.update(entropy_cost_param=_to(device, np.array([cfg['entropy_cost_param']], np.float32)),
              d_entropy_cost_param=bufs['d_ecp'][1], entropy_cost_adjustment_speed=cfg['entropy_cost_adjustment_speed'],
              target_entropy=share)
  else:
    kw.update(entropy_cost=cfg['entropy_cost'])
  d_head = bufs['d_head'][1]
  ops.normal_tanh_loss_fwd_bwd(head, ld, head[2 * D:], ld, _to(device, inp['beh']), _to(device, inp['actions']),
                               _to(device, inp['noise']), _to(device, inp['rewards']), ops.as_u8(_to(device, inp['done'])),
                               T, B, D, d_head, d_head[2 * D:], bufs['scalars'][1], ws, bufs['vs'][1], bufs['pg'][1], **kw)
  torch.cuda.synchronize()
  for name, (big, _) in list(bufs.items()) + [('workspace', (ws_big, ws))]:
    assert _intact(big), 'guard of %s overwritten' % name
  dh = d_head.cpu().numpy().reshape(T + 1, B, ld)
  return dict(d_head=dh, d_params=dh[..., :2 * D], d_baseline=dh[..., 2 * D], vs=bufs['vs'][1].cpu().numpy().reshape(T, B),
              pg=bufs['pg'][1].cpu().numpy().reshape(T, B), scalars=bufs['scalars'][1].cpu().numpy()[:13],
              scalars_all=bufs['scalars'][1].cpu().numpy(),
              d_entropy_cost_param=float(bufs['d_ecp'][1][0]) if 'entropy_cost_param' in cfg else None)


def _cfgs():
  out = []
  for adaptive, kl, mar in itertools.product((False, True), (0.0, 0.1), (0.0, 1.0)):
    c = dict(kl_cost=kl, max_abs_reward=mar)
    if adaptive:
      c.update(entropy_cost_param=-0.4, entropy_cost_adjustment_speed=10.0, target_entropy=-1.5 if kl else None)
    else:
      c.update(entropy_cost=0.01)
    out.append(pytest.param(c, id='%s-kl%g-mar%g' % ('adaptive' if adaptive else 'fixed', kl, mar)))
  return out


@pytest.mark.parametrize('cfg', _cfgs())
@pytest.mark.parametrize('D', [1, 6, 17, 64], ids=lambda d: 'D%d' % d)
@pytest.mark.parametrize('B', [3, 32, 512], ids=lambda b: 'B%d' % b)
def test_kernel_vs_oracle(device, B, D, cfg):
  """T = 20; scalars, vs, pg_advantages, d_params, d_baseline: the kernel's distance to the fp64 oracle is at most twice
  the fp32 oracle's, plus the floors of normal_tanh_oracle.gate (README: 'held to an fp64 evaluation at <= 2x torch's
  fp32 error').  Containment: guards intact, every in-range element overwritten, pad columns untouched."""
  T = 20
  inp = nto.make_inputs(1000 * B + D, T, B, D)
  r32, r64 = nto.evaluate(inp, torch.float32, **cfg), nto.evaluate(inp, torch.float64, **cfg)
  for r in (r32, r64):                                 # the gate rests on a finite fp32 oracle
    assert all(np.all(np.isfinite(r[k])) for k in ('scalars', 'vs', 'pg', 'd_params', 'd_baseline'))
  got = _kernel(device, inp, cfg, T, B)
  res = nto.gate(got, r32, r64)
  print('GATE B=%d D=%d %s' % (B, D, ' '.join('%s=%.3g/%.3g(x%.2f)' % ((k,) + v) for k, v in res.items())))
  for k, (dist, allowed, _) in res.items():
    assert dist <= allowed, (k, dist, allowed)
  if got['d_entropy_cost_param'] is not None:
    ref = r64['d_entropy_cost_param']
    assert abs(got['d_entropy_cost_param'] - ref) <= 2 * abs(r32['d_entropy_cost_param'] - ref) + 2e-5 * max(1.0, abs(ref))
  dh = got['d_head']
  assert np.all(dh[..., 2 * D + 1:] == FILL)                                   # pad columns: not written
  assert not np.any(dh[..., :2 * D + 1] == FILL)                               # everything in range: overwritten
  assert np.all(dh[-1, :, :2 * D + 1] == 0.0)                                  # bootstrap row: zeros
  assert not np.any(got['vs'] == FILL) and not np.any(got['pg'] == FILL)
  assert np.all(got['scalars_all'][13:] == FILL) and not np.any(got['scalars'] == FILL)
  assert got['scalars'][9] == np.abs(inp['actions'][:-1]).max()


def test_replica_shares(device):
  """Two column shards with mean_denominator = T * B_global (and their share of the target entropy) sum to the
  full-batch loss, parameter-cost gradient and head gradients."""
  T, B, D = 20, 64, 6
  cfg = dict(kl_cost=0.1, max_abs_reward=0.0, entropy_cost_param=-0.6, entropy_cost_adjustment_speed=10.0,
             target_entropy=-1.1)
  inp = nto.make_inputs(5, T, B, D)
  full = _kernel(device, inp, cfg, T, B)
  parts = []
  for sl in (slice(0, 32), slice(32, 64)):
    sub = dict((k, np.ascontiguousarray(v[:, sl]) if isinstance(v, np.ndarray) else v) for k, v in inp.items())
    parts.append(_kernel(device, sub, cfg, T, 32, mean_denominator=T * B))
  tot = parts[0]['scalars'][0] + parts[1]['scalars'][0]
  assert abs(tot - full['scalars'][0]) < 1e-5 * max(1.0, abs(full['scalars'][0]))
  g = parts[0]['d_entropy_cost_param'] + parts[1]['d_entropy_cost_param']
  assert abs(g - full['d_entropy_cost_param']) <= 1e-5 * max(abs(full['d_entropy_cost_param']), 1e-3)
  assert abs(parts[0]['scalars'][12] + parts[1]['scalars'][12] - full['scalars'][12]) < 1e-5      # policy/std shares
  np.testing.assert_allclose(np.concatenate([p['d_params'] for p in parts], 1), full['d_params'], rtol=1e-5, atol=1e-8)
  np.testing.assert_allclose(np.concatenate([p['d_baseline'] for p in parts], 1), full['d_baseline'], rtol=1e-5, atol=1e-8)


def test_log_prob_entropy_match_oracle(device):
  from seed_rl_amd import parametric_distribution as pd
  inp = nto.make_inputs(9, 6, 5, 17)
  dist = pd.normal_tanh_distribution(17)
  params, act, eps = _to(device, inp['beh'][:-1]), _to(device, inp['actions'][:-1]), _to(device, inp['noise'])
  lp, ent = dist.log_prob(params, act), dist.entropy(params, eps)
  p64 = torch.tensor(inp['beh'][:-1]).double()
  np.testing.assert_allclose(lp.cpu().numpy(), nto.log_prob(p64, torch.tensor(inp['actions'][:-1])).numpy(), rtol=2e-6, atol=2e-6)
  np.testing.assert_allclose(ent.cpu().numpy(), nto.entropy(p64, torch.tensor(inp['noise'])).numpy(), rtol=1e-5, atol=1e-5)
  assert lp.shape == (6, 5) and ent.shape == (6, 5)
  dist.seed_noise(4)
  e1 = dist.entropy(params)
  dist.seed_noise(4)
  assert torch.equal(e1, dist.entropy(params)) and not torch.equal(e1, dist.entropy(params))


def test_sampling(device):
  from seed_rl_amd import ops, parametric_distribution as pd
  rows, D = 1 << 16, 3
  loc, s = np.array([0.3, -0.5, 0.0]), np.array([0.0, -1.0, 0.5])
  params = _to(device, np.tile(np.concatenate([loc, s]).astype(np.float32), (rows, 1)))
  dist = pd.normal_tanh_distribution(D)
  a0 = dist.sample(params, seed=3)
  a1 = dist.sample(params)                              # the counter moved on
  assert a0.shape == (rows, D) and a0.dtype == torch.float32
  assert torch.equal(a0, dist.sample(params, seed=3)) and not torch.equal(a0, a1)
  assert float(a0.abs().max()) <= 1.0 and float(a1.abs().max()) <= 1.0
  # equal (seed, counter) give equal actions; the call advances the counter by one
  rng = torch.tensor([3, 1], dtype=torch.int64, device=device)
  out = torch.empty((rows, D), dtype=torch.float32, device=device)
  ops.normal_tanh_sample(params, 2 * D, rows, D, rng, out)
  assert torch.equal(out, a1) and rng.tolist() == [3, 2]
  # strided parameter rows (a head-GEMM output) give the same draws
  wide = torch.zeros((rows, 8), dtype=torch.float32, device=device)
  wide[:, :2 * D] = params
  assert torch.equal(dist.sample_rows(wide, 8, rows, torch.tensor([3, 0], dtype=torch.int64, device=device)), a0)
  # moments of atanh(a): N(loc, sigma^2) within 4 standard errors
  x = torch.atanh(a0.double()).cpu().numpy()
  sigma = np.log1p(np.exp(s)) + 1e-3
  assert np.all(np.isfinite(x))
  assert np.all(np.abs(x.mean(0) - loc) <= 4 * sigma / np.sqrt(rows))
  assert np.all(np.abs(x.var(0, ddof=1) - sigma ** 2) <= 4 * sigma ** 2 * np.sqrt(2.0 / (rows - 1)))
  # the standard-normal fill the learner draws its entropy noise with
  n = dist.draw_noise((rows, 5), device).double().cpu().numpy().ravel()
  assert abs(n.mean()) <= 4 / np.sqrt(n.size) and abs(n.var() - 1) <= 4 * np.sqrt(2.0 / n.size)


MLP, LSTM, OBS = (64, 32), (64,), 17


def _unroll_inputs(rng, T1, B, D):
  beh = (0.3 * rng.normal(size=(T1, B, 2 * D))).astype(np.float32)
  sig = np.log1p(np.exp(beh[..., D:].astype(np.float64))) + 1e-3
  return dict(actions=np.tanh(beh[..., :D] + sig * rng.normal(size=(T1, B, D))).astype(np.float32), beh=beh,
              reward=rng.normal(size=(T1, B)).astype(np.float32), done=rng.uniform(size=(T1, B)) < 0.15,
              prev=np.zeros((T1, B, D), np.float32), obs=rng.normal(size=(T1, B, OBS)).astype(np.float32),
              state=[((0.1 * rng.normal(size=(B, h))).astype(np.float32), (0.1 * rng.normal(size=(B, h))).astype(np.float32))
                     for h in LSTM])


def _make_learner(device, u, D, capturable=False):
  from seed_rl_amd import learner, networks, optimizers, utils, parametric_distribution as pd
  dist = pd.normal_tanh_distribution(D)
  agent = networks.MLPandLSTM(dist, OBS, MLP, LSTM, device=device, seed=6)
  lrn = learner.Learner(agent, optimizers.Adam(1e-3, capturable=capturable), dist)
  env = utils.EnvOutput(_to(device, u['reward']), _to(device, u['done']), _to(device, u['obs']), None, None)
  ao = networks.AgentOutput(_to(device, u['actions']), _to(device, u['beh']), _to(device, u['reward'] * 0.5))
  dstate = tuple((_to(device, h), _to(device, c)) for h, c in u['state'])
  return dist, agent, lrn, learner.Unroll(dstate, _to(device, u['prev']), env, ao)


def test_mlp_and_lstm_continuous_train_step_parity(device):
  """MLPandLSTM(normal_tanh_distribution(6), ...): bit-identical initialisation with the oracle network whose policy
  head is 2 D wide, head outputs / gradients / loss of one step against nets_torch.mlp_lstm_unroll + the oracle head."""
  T1, B, D = 7, 5, 6
  u = _unroll_inputs(np.random.default_rng(5), T1, B, D)
  dist, agent, lrn, unroll = _make_learner(device, u, D)
  ref = nets_torch.init_params(nets_torch.param_spec('mlp_lstm', 2 * D, core=(OBS, MLP, LSTM)), seed=6)
  for (n, v) in agent.trainable_variables:
    if n != 'entropy_cost_param':
      np.testing.assert_array_equal(v.cpu().numpy(), ref[n])
  dist.seed_noise(11)
  noise = dist.draw_noise((T1 - 1, B, D), device).cpu()
  dist.seed_noise(11)                                   # the step below draws the very same noise
  loss, session = lrn.compute_gradients(unroll)
  p = nets_torch.to_torch(ref, requires_grad=True)
  t = lambda a: torch.tensor(a)
  params, baseline, _ = nets_torch.mlp_lstm_unroll(p, len(MLP), len(LSTM), t(u['obs']), t(u['done']),
                                                   [(t(h), t(c)) for h, c in u['state']])
  total, out, _, _ = nto.loss(params, baseline, t(u['beh']), t(u['actions']), noise, t(u['reward']), t(u['done']))
  total.backward()
  head, _, ldh = agent.head_buffers()
  head = head.cpu().numpy().reshape(T1, B, ldh)
  print('PARITY head %.3g loss %.8g vs %.8g' % (np.max(np.abs(head[..., :2 * D] - params.detach().numpy())), float(loss),
                                                 float(total)))
  assert np.max(np.abs(head[..., :2 * D] - params.detach().numpy())) < 2e-4
  assert np.max(np.abs(head[..., 2 * D] - baseline.detach().numpy())) < 2e-4
  assert abs(float(loss) - float(total)) <= 2e-5 * max(1.0, abs(float(total)))
  assert abs(float(session['policy/std']) - float(out['policy_std'])) < 1e-5
  grads = agent.reference_gradients()
  for n, tt in p.items():
    g, r = grads[n].cpu().numpy(), tt.grad.numpy()
    assert np.max(np.abs(g - r)) <= 1e-3 * max(np.abs(r).max(), 1e-3), n
  # actions of the agent itself: float32 [.., D] from distribution.sample
  out1, _ = agent(unroll.prev_actions, unroll.env_outputs, unroll.agent_state, unroll=True)
  assert out1.action.shape == (T1, B, D) and out1.action.dtype == torch.float32 and float(out1.action.abs().max()) <= 1.0
  assert out1.policy_logits.shape == (T1, B, 2 * D)


def test_graphed_step_matches_eager_continuous(device):
  """Two replays of the captured step == two eager steps, bitwise (as tests/test_gpu_graph.py holds the categorical head
  to), with the entropy noise drawn inside the graph from the same generator state."""
  from seed_rl_amd import learner
  T1, B, D = 7, 5, 6
  u = _unroll_inputs(np.random.default_rng(5), T1, B, D)
  dist, agent, eager, unroll = _make_learner(device, u, D, capturable=True)
  dist.seed_noise(21)
  losses = [float(eager.minimize(unroll)[0]) for _ in range(2)]
  dist2, agent2, graphed, unroll2 = _make_learner(device, u, D, capturable=True)
  p0 = agent2.flat.params.clone()
  step = learner.GraphedStep(graphed, unroll2, warmup=2)
  assert graphed.optimizer.iterations == 0 and torch.equal(agent2.flat.params, p0)
  dist2.seed_noise(21)                                  # the warm-up steps drew noise: back to the eager run's state
  glosses = []
  for _ in range(2):
    out = step()
    torch.cuda.synchronize()
    glosses.append(float(out[0]))
  assert glosses == losses
  assert torch.equal(agent2.flat.params, agent.flat.params)
  step.check_errors()


def test_central_inference_refuses_continuous_actions(device):
  from seed_rl_amd import inference, networks, parametric_distribution as pd
  agent = networks.MLPandLSTM(pd.normal_tanh_distribution(3), 8, (16,), (16,), device=device)
  with pytest.raises(NotImplementedError, match='scalar int64 actions'):
    inference.InferenceState(agent, 4, 5, None, None, None)
  with pytest.raises(NotImplementedError, match='scalar int64 actions'):
    inference.FusedInferenceState(agent, 4, 5, None, None, 4)
