"""Oracle of the tanh-Gaussian V-trace loss head: a restatement, in our own words and with torch on the CPU, of
common/parametric_distribution.py:124-202 (TanhTransformedDistribution over tfd.Normal, softplus_default_std_fn,
tfd.Independent) and of the distribution-agnostic loss of agents/vtrace/learner.py:82-157.  Every gradient comes from
autograd; the dtype of the inputs decides whether it is the fp32 or the fp64 evaluation.

TensorFlow Probability is not installed here, so this is "parity unpinned" like the Keras layers of oracle/nets_torch:
nothing below was checked against a TFP run.  The one fact pinned to the reference is the additivity its joint test
relies on (common/parametric_distribution_test.py:50-84), asserted in tests/test_normal_tanh_host.py.

Conventions that the reference leaves to its fp32 graph and that both precisions share here, so that they evaluate
the same function: the clip threshold is float32(0.999) (the action tensor is fp32 and is compared with it), and
log(1 - threshold) is taken of the Python floats, as `tf.math.log(1. - threshold)` is.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets_torch

THRESHOLD = float(np.float32(.999))
LOG_EPSILON = math.log(1. - .999)
MIN_STD = 1e-3


def split(parameters):
  d = parameters.shape[-1] // 2
  return parameters[..., :d], F.softplus(parameters[..., d:]) + MIN_STD      # loc, sigma (:187-188, :196-197)


def fldj(x):
  """tfp.bijectors.Tanh forward log-det-Jacobian."""
  return 2. * (math.log(2.) - x - F.softplus(-2. * x))


def log_prob(parameters, actions):
  """:156-165 over :198-200; actions [.., D] in [-1, 1]; returns [..]."""
  loc, sigma = split(parameters)
  a = actions.to(parameters.dtype)
  thr = THRESHOLD
  x0 = math.atanh(thr)
  left = torch.special.log_ndtr((-x0 - loc) / sigma) - LOG_EPSILON           # log_cdf(-atanh thr) - log eps (:151-152)
  right = torch.special.log_ndtr(-(x0 - loc) / sigma) - LOG_EPSILON          # log_survival_function(atanh thr) (:153-154)
  ac = torch.clamp(a, -thr, thr)                                             # :159
  x = torch.atanh(ac)
  z = (x - loc) / sigma
  inner = -0.5 * z * z - torch.log(sigma) - 0.5 * math.log(2. * math.pi) - fldj(x)
  lp = torch.where(ac <= -thr, left, torch.where(ac >= thr, right, inner))   # :162-165
  return lp.sum(-1)                                                          # tfd.Independent


def entropy(parameters, noise):
  """:173-177: Normal entropy + the Jacobian at ONE sample loc + sigma * noise; summed over D."""
  loc, sigma = split(parameters)
  return (0.5 * math.log(2. * math.pi * math.e) + torch.log(sigma) + fldj(loc + sigma * noise.to(parameters.dtype))).sum(-1)


SCALARS = ('total', 'policy', 'v', 'entropy_loss', 'kl', 'entropy_mean', 'kl_mean', 'value_mean', 'v_l2_error',
           'max_action_abs', 'entropy_cost', 'entropy_adjustment', 'policy_std')    # SEEDHIP_LOSS_* slots 0..12


def loss(params, baseline, beh_params, actions, noise, rewards, done, entropy_cost=0.00025, baseline_cost=0.5,
         kl_cost=0.0, discounting=0.99, lambda_=1.0, max_abs_reward=0.0, entropy_cost_param=None,
         entropy_cost_adjustment_speed=10.0, target_entropy=None, mean_denominator=None):
  """learner.py:82-157 with every reduce_mean written as sum / mean_denominator (T * B by default; the global T * B for
  a column shard, whose target_entropy is then its share).  Returns (total, {name: 0-d tensor}, vs, pg)."""
  T, B = rewards.shape[0] - 1, rewards.shape[1]
  n = float(mean_denominator or T * B)
  dt = params.dtype
  vals, bootstrap = baseline[:-1], baseline[-1]
  rew, dn = rewards[1:].to(dt), done[1:]
  if max_abs_reward:
    rew = torch.clamp(rew, -max_abs_reward, max_abs_reward)
  disc = (~dn).to(dt) * discounting
  tlp = log_prob(params[:-1], actions[:-1])
  blp = log_prob(beh_params[:-1].to(dt), actions[:-1])
  vs, pg = nets_torch.vtrace_torch(tlp, blp, disc, rew, vals, bootstrap, lambda_=lambda_)
  policy_loss = -(tlp * pg).sum() / n
  mse = ((vs - vals) ** 2).sum() / n
  v_loss = baseline_cost * 0.5 * mse
  ent = entropy(params[:-1], noise).sum() / n
  kl_mean = (blp - tlp).sum() / n
  kl_loss = kl_cost * kl_mean
  adjustment = torch.zeros((), dtype=dt)
  cost = torch.tensor(float(entropy_cost), dtype=dt)
  if entropy_cost_param is not None:
    c = torch.exp(entropy_cost_adjustment_speed * entropy_cost_param)
    cost = c.detach()
    adjustment = c * (ent.detach() - target_entropy) if target_entropy else 0. * c
  entropy_loss = cost * -ent
  total = policy_loss + v_loss + entropy_loss + kl_loss + adjustment
  D = actions.shape[-1]
  out = dict(total=total, policy=policy_loss, v=v_loss, entropy_loss=entropy_loss, kl=kl_loss, entropy_mean=ent,
             kl_mean=kl_mean, value_mean=vals.sum() / n, v_l2_error=torch.sqrt(mse),
             max_action_abs=actions[:-1].abs().max().to(dt), entropy_cost=cost, entropy_adjustment=adjustment,
             policy_std=split(params[:-1])[1].sum() / (n * D))
  return total, out, vs, pg


# --------------------------------------------------------------------------------------------------------------------- #
# Seeded inputs of the kernel-vs-oracle tests and the gate both of them apply.
# --------------------------------------------------------------------------------------------------------------------- #
def make_inputs(seed, T, B, D, ld=None, perturb=0.05):
  """loc ~ U[-2, 2], s ~ U[-1, 1]; target = behaviour + N(0, perturb^2); actions tanh(loc_b + sigma_b eps) in fp32 with
  about 5 % of the elements set to exactly +-1.0, +-0.999 and +-0.9989999 (both clipped ends and the last interior
  value).  `head` is the learner's head-GEMM row layout [params(2 D) | baseline | pad] of stride ld."""
  rng = np.random.default_rng(seed)
  T1 = T + 1
  ld = ld or (2 * D + 1 + 3) // 4 * 4
  beh = np.concatenate([rng.uniform(-2, 2, (T1, B, D)), rng.uniform(-1, 1, (T1, B, D))], -1).astype(np.float32)
  tgt = (beh + perturb * rng.standard_normal(beh.shape)).astype(np.float32)
  sig = np.log1p(np.exp(beh[..., D:].astype(np.float64))) + MIN_STD
  act = np.tanh(beh[..., :D] + sig * rng.standard_normal((T1, B, D))).astype(np.float32)
  special = np.array([1.0, -1.0, 0.999, -0.999, 0.9989999, -0.9989999], np.float32)
  hit = rng.uniform(size=act.shape) < 0.05
  act[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
  head = np.zeros((T1, B, ld), np.float32)
  head[..., :2 * D] = tgt
  head[..., 2 * D] = rng.standard_normal((T1, B)).astype(np.float32)
  return dict(head=head, beh=beh, actions=act, noise=rng.standard_normal((T, B, D)).astype(np.float32),
              rewards=rng.standard_normal((T1, B)).astype(np.float32), done=rng.uniform(size=(T1, B)) < 0.1, D=D, ld=ld)


def evaluate(inp, dtype, entropy_cost_param=None, **cfg):
  """The oracle on make_inputs() in `dtype`: dict(scalars [13], vs, pg, d_params [T+1, B, 2 D], d_baseline [T+1, B],
  d_entropy_cost_param) as float64 numpy arrays."""
  D = inp['D']
  params = torch.tensor(inp['head'][..., :2 * D]).to(dtype).requires_grad_(True)
  baseline = torch.tensor(inp['head'][..., 2 * D]).to(dtype).requires_grad_(True)
  ecp = None
  if entropy_cost_param is not None:
    ecp = torch.tensor(float(np.float32(entropy_cost_param)), dtype=dtype, requires_grad=True)
  total, out, vs, pg = loss(params, baseline, torch.tensor(inp['beh']), torch.tensor(inp['actions']),
                            torch.tensor(inp['noise']), torch.tensor(inp['rewards']), torch.tensor(inp['done']),
                            entropy_cost_param=ecp, **cfg)
  total.backward()
  f = lambda t: t.detach().double().numpy()
  return dict(scalars=np.array([float(out[k].detach()) for k in SCALARS]), vs=f(vs), pg=f(pg), d_params=f(params.grad),
              d_baseline=f(baseline.grad), d_entropy_cost_param=None if ecp is None else float(ecp.grad))


def gate(got, ref32, ref64):
  """The project's rule (README: 'held to an fp64 evaluation at <= 2x torch's fp32 error'), per tensor on the maximum
  absolute distance: |got - fp64| <= 2 |fp32 oracle - fp64| + floor.  Floors: gradients 1e-7 (the categorical loss
  tests' atol); losses and logged scalars 2e-5 * max(1, |value|) (their loss bound); vs / pg_advantages
  1e-6 * max(1, max |value|) (the V-trace tests' rtol = atol = 1e-6 of the reference's own test).
  Returns {name: (distance, allowed, distance / fp32 oracle's distance)}; the caller prints, then asserts."""
  res = {}
  for name in ('scalars', 'vs', 'pg', 'd_params', 'd_baseline'):
    g, r32, r64 = (np.asarray(x[name], np.float64) for x in (got, ref32, ref64))
    if name == 'scalars':
      floor = 2e-5 * np.maximum(1.0, np.abs(r64))
      dist, d32 = np.abs(g - r64), np.abs(r32 - r64)
      worst = int(np.argmax(dist - (2 * d32 + floor)))
      res[name] = (float(dist[worst]), float(2 * d32[worst] + floor[worst]), float(dist.max() / max(d32.max(), 1e-30)))
      continue
    floor = 1e-7 if name.startswith('d_') else 1e-6 * max(1.0, float(np.abs(r64).max()))
    dist, d32 = float(np.abs(g - r64).max()), float(np.abs(r32 - r64).max())
    res[name] = (dist, 2 * d32 + floor, dist / max(d32, 1e-30))
  return res
