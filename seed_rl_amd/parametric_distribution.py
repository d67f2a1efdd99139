"""Action distributions on MI355X: categorical (Discrete spaces) and tanh-Gaussian (Box spaces).

Mirrors /root/reference/common/parametric_distribution.py (ParametricDistribution
:31-80, categorical_distribution :83-97, TanhTransformedDistribution / normal_tanh_distribution :124-202,
get_parametric_distribution_for_action_space :293-332): `log_prob(parameters, actions)` and
`entropy(parameters)` run as one HIP kernel each (csrc/loss.hip `seedhip_categorical_log_prob_entropy`,
csrc/loss_normal_tanh.hip `seedhip_normal_tanh_log_prob_entropy`).  Every distribution names the fused loss
head the learner runs for it (`loss_head`).  MultiDiscrete / Tuple spaces, the ClippedIdentity
post-processor and the shifted std functions of the reference (:100-120, :205-275) are not built.
"""
import torch

from seed_rl_amd import _lib


class ParametricDistribution(object):
  """Categorical distribution over `param_size` actions (logits parametrisation)."""

  loss_head = 'categorical'          # which fused loss head learner.compute_loss runs (learner.LOSS_HEADS)

  def __init__(self, param_size, dtype=torch.int64):
    self._param_size = param_size
    self._dtype = dtype
    self._rng = {}

  @property
  def param_size(self):
    return self._param_size

  @property
  def reparametrizable(self):
    return False

  def _rows(self, parameters):
    if parameters.shape[-1] != self._param_size:
      raise ValueError('expected last dim %d, got %s' % (self._param_size, tuple(parameters.shape)))
    return parameters.reshape(-1, self._param_size).to(torch.float32).contiguous()

  def _run(self, parameters, actions, want_lp, want_ent):
    _lib.require_cuda(parameters)
    with torch.no_grad():
      logits = self._rows(parameters)
      rows = logits.shape[0]
      lp = torch.empty(rows, device=logits.device, dtype=torch.float32) if want_lp else None
      ent = torch.empty(rows, device=logits.device, dtype=torch.float32) if want_ent else None
      act = None
      esz = 0
      if actions is not None:
        if tuple(actions.shape) != tuple(parameters.shape[:-1]):
          raise ValueError('actions shape %s != %s' % (tuple(actions.shape), tuple(parameters.shape[:-1])))
        act = actions.reshape(-1)
        if act.dtype not in (torch.int32, torch.int64):
          act = act.to(torch.int64)
        act = act.contiguous()
        esz = act.element_size()
      with torch.cuda.device(logits.device):
        rc = _lib.lib().seedhip_categorical_log_prob_entropy(
            _lib.ptr(logits), _lib.ptr(act), esz, rows, self._param_size, _lib.ptr(lp), _lib.ptr(ent),
            _lib.stream())
      _lib.check(rc, 'seedhip_categorical_log_prob_entropy')
    shp = parameters.shape[:-1]
    return (lp.reshape(shp) if want_lp else None, ent.reshape(shp) if want_ent else None)

  def log_prob(self, parameters, actions):
    """parametric_distribution.py:69-70."""
    return self._run(parameters, actions, True, False)[0]

  def entropy(self, parameters):
    """parametric_distribution.py:72-74."""
    return self._run(parameters, None, False, True)[1]

  def sample(self, parameters, seed=None):
    """parametric_distribution.py:66-67 (tfd.Categorical.sample; used by the agents' _head,
    dmlab/networks.py:120-122): Gumbel-max over counter-based randoms in one kernel (csrc/inference.hip:
    seedhip_categorical_sample); the generator state is a device (seed, counter) pair per device."""
    _lib.require_cuda(parameters)
    from seed_rl_amd import ops
    logits = self._rows(parameters)
    key = logits.device
    rng = self._rng.get(key)
    if rng is None or seed is not None:
      rng = torch.tensor([0x5EED if seed is None else int(seed), 0], dtype=torch.int64, device=logits.device)
      self._rng[key] = rng
    out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
    ops.categorical_sample(logits, self._param_size, logits.shape[0], self._param_size, rng, out)
    return out.reshape(parameters.shape[:-1]).to(self._dtype)


def categorical_distribution(n_actions, dtype=torch.int64):
  """parametric_distribution.py:83-97."""
  return ParametricDistribution(n_actions, dtype)


class NormalTanhDistribution(object):
  """tanh(Normal(loc, softplus(s) + 1e-3)) per action dimension, independent over D (parametric_distribution.py:124-202):
  parameters [.., 2 D] = [loc | s], actions float32 [.., D] in [-1, 1].  log_prob clips the action to +-0.999 and gives
  the clipped ends their averaged tail mass; entropy is the reference's single-sample estimate, whose standard-normal
  draws come from `noise` or from this object's own device generator (seed_noise / draw_noise)."""

  loss_head = 'normal_tanh'

  def __init__(self, num_actions):
    if not 1 <= int(num_actions) <= 64:
      raise ValueError('normal_tanh_distribution: 1 <= num_actions <= 64, got %r' % (num_actions,))
    self._d = int(num_actions)
    self._rng = {}          # device -> (seed, counter) of sample()
    self._noise_rng = {}    # device -> (seed, counter) of the entropy noise
    self._noise_seed = 0xE17

  @property
  def param_size(self):
    return 2 * self._d

  @property
  def num_actions(self):
    return self._d

  @property
  def reparametrizable(self):
    return True

  def _rows(self, parameters):
    if parameters.shape[-1] != 2 * self._d:
      raise ValueError('expected last dim %d, got %s' % (2 * self._d, tuple(parameters.shape)))
    return parameters.reshape(-1, 2 * self._d).to(torch.float32).contiguous()

  def _like_actions(self, t, parameters, what):
    if tuple(t.shape) != tuple(parameters.shape[:-1]) + (self._d,):
      raise ValueError('%s shape %s != %s' % (what, tuple(t.shape), tuple(parameters.shape[:-1]) + (self._d,)))
    return t.reshape(-1, self._d).to(torch.float32).contiguous()

  def _state(self, table, device, seed):
    rng = table.get(device)
    if rng is None:
      rng = torch.tensor([int(seed), 0], dtype=torch.int64, device=device)
      table[device] = rng
    return rng

  # -- entropy noise: a seedable device generator (one (seed, counter) pair per device; the fill kernel advances the
  # counter itself, so drawing sits inside captured HIP graphs) ------------------------------------------------------- #
  def seed_noise(self, seed):
    """Restarts the entropy-noise stream at (seed, 0), IN PLACE where a state exists: a captured graph holds its address."""
    self._noise_seed = int(seed)
    for rng in self._noise_rng.values():
      rng.copy_(torch.tensor([int(seed), 0], dtype=torch.int64))

  def draw_noise(self, shape, device, out=None):
    """Standard-normal float32 `shape` from the noise stream (advances it by one call)."""
    from seed_rl_amd import ops
    device = torch.device(device)
    if out is None:
      out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    ops.normal_fill(out, self._state(self._noise_rng, device, self._noise_seed))
    return out

  def _run(self, parameters, actions, noise, want_lp, want_ent):
    from seed_rl_amd import ops
    _lib.require_cuda(parameters)
    with torch.no_grad():
      params = self._rows(parameters)
      rows = params.shape[0]
      lp = torch.empty(rows, device=params.device, dtype=torch.float32) if want_lp else None
      ent = torch.empty(rows, device=params.device, dtype=torch.float32) if want_ent else None
      act = self._like_actions(actions, parameters, 'actions') if want_lp else None
      if want_ent:
        eps = (self.draw_noise((rows, self._d), params.device) if noise is None
               else self._like_actions(noise, parameters, 'noise'))
      else:
        eps = None
      ops.normal_tanh_log_prob_entropy(params, act, eps, rows, self._d, lp, ent)
    shp = parameters.shape[:-1]
    return (lp.reshape(shp) if want_lp else None, ent.reshape(shp) if want_ent else None)

  def log_prob(self, parameters, actions):
    """parametric_distribution.py:69-70 over :156-165."""
    return self._run(parameters, actions, None, True, False)[0]

  def entropy(self, parameters, noise=None):
    """parametric_distribution.py:72-74 over :173-177 (single-sample estimate)."""
    return self._run(parameters, None, noise, False, True)[1]

  def sample_rows(self, rows_params, ld, rows, rng_state):
    """actions float32 [rows, D] for parameter rows of stride ld (a head-GEMM output read in place)."""
    from seed_rl_amd import ops
    out = torch.empty((rows, self._d), dtype=torch.float32, device=rows_params.device)
    ops.normal_tanh_sample(rows_params, ld, rows, self._d, rng_state, out)
    return out

  def sample(self, parameters, seed=None):
    """parametric_distribution.py:66-67: tanh(loc + sigma * eps), eps from counter-based randoms
    (seedhip_normal_tanh_sample); equal (seed, counter) give equal actions."""
    _lib.require_cuda(parameters)
    params = self._rows(parameters)
    if seed is not None:
      self._rng.pop(params.device, None)
    rng = self._state(self._rng, params.device, 0x5EED if seed is None else seed)
    return self.sample_rows(params, 2 * self._d, params.shape[0], rng).reshape(tuple(parameters.shape[:-1]) + (self._d,))


def normal_tanh_distribution(num_actions):
  """parametric_distribution.py:191-202 with the default softplus_default_std_fn (other std functions: not built)."""
  return NormalTanhDistribution(num_actions)


class Discrete(object):
  """Minimal stand-in for gym.spaces.Discrete (gym is not part of the hot path)."""

  def __init__(self, n, dtype=torch.int64):
    self.n = n
    self.dtype = dtype


class Box(object):
  """Minimal stand-in for gym.spaces.Box: per-dimension bounds `low` / `high` of one shape."""

  def __init__(self, low, high, shape=None, dtype=torch.float32):
    import numpy as np
    if shape is None:
      shape = np.broadcast(np.asarray(low), np.asarray(high)).shape
    self.shape = tuple(shape)
    self.low = np.broadcast_to(np.asarray(low, np.float64), self.shape)
    self.high = np.broadcast_to(np.asarray(high, np.float64), self.shape)
    self.dtype = dtype


def check_box_space(space):
  """parametric_distribution.py:283-290."""
  assert len(space.shape) == 1, space.shape
  if any(l != -1 for l in space.low):
    raise ValueError('Learner only supports actions bounded to [-1,1]: %s' % (space.low,))
  if any(h != 1 for h in space.high):
    raise ValueError('Learner only supports actions bounded to [-1,1]: %s' % (space.high,))


def get_parametric_distribution_for_action_space(action_space, continuous_config=None):
  """parametric_distribution.py:293-332: Discrete -> categorical (:306-307), Box -> tanh-Gaussian with the default
  softplus std (:310-317)."""
  if isinstance(action_space, Discrete) or hasattr(action_space, 'n'):
    return categorical_distribution(action_space.n, getattr(action_space, 'dtype', torch.int64))
  if isinstance(action_space, Box) or (hasattr(action_space, 'low') and hasattr(action_space, 'high')):
    check_box_space(action_space)
    if continuous_config is not None:
      raise NotImplementedError('continuous_config: the ClippedIdentity post-processor and the shifted std functions '
                                '(safe_exp / shifted softplus) are not built; only Tanh with softplus_default_std_fn is')
    return normal_tanh_distribution(action_space.shape[0])
  raise NotImplementedError('%s: MultiDiscrete and Tuple action spaces, the ClippedIdentity post-processor and the '
                            'shifted std functions are not built; Discrete and Box([-1, 1]) are'
                            % type(action_space).__name__)
