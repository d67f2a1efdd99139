"""IMPALA / V-trace learner step on MI355X.

Mirrors /root/reference/agents/vtrace/learner.py on the hot path:
  * `Unroll`                       learner.py:162-163
  * loss hyper-parameters          learner.py:51-62 (absl flags -> LossConfig)
  * `compute_loss(...)`            learner.py:73-159 (same positional signature)
  * `Learner.minimize(unroll)`     learner.py:255-280 (compute_gradients +
                                   apply_gradients; the cross-replica gradient SUM the
                                   Keras optimizer does implicitly on TPU becomes one
                                   RCCL all-reduce of the flat gradient bucket)
The control plane of learner_loop (gRPC server, checkpoint manager, logger thread,
tf.data pipeline; learner.py:170-483) is out of scope.
"""
import collections

import torch

from seed_rl_amd import ops

Unroll = collections.namedtuple('Unroll', 'agent_state prev_actions env_outputs agent_outputs')


class LossConfig(object):
  """Flag defaults of agents/vtrace/learner.py:51-62."""

  def __init__(self, entropy_cost=0.00025, target_entropy=None, entropy_cost_adjustment_speed=10.,
               baseline_cost=.5, kl_cost=0., discounting=.99, lambda_=1., max_abs_reward=0.):
    self.entropy_cost = entropy_cost
    self.target_entropy = target_entropy
    self.entropy_cost_adjustment_speed = entropy_cost_adjustment_speed
    self.baseline_cost = baseline_cost
    self.kl_cost = kl_cost
    self.discounting = discounting
    self.lambda_ = lambda_
    self.max_abs_reward = max_abs_reward


LOGGED = collections.OrderedDict([      # logger.log names of learner.py:138-157 -> scalars[] index
    ('V/value function', 7), ('V/L2 error', 8), ('losses/policy', 1), ('losses/V', 2),
    ('losses/entropy', 3), ('losses/kl', 4), ('losses/total', 0),
    ('policy/max_action_abs(before_tanh)', 9), ('policy/entropy', 5), ('policy/kl(old|new)', 6)])


class DictLogger(object):
  """Stand-in for utils.ProgressLogger's log_session()/log() (utils.py:546-677)."""

  def log_session(self):
    return collections.OrderedDict()

  def log(self, session, name, value):
    session[name] = value


def _categorical_loss_head(dist, agent, agent_outputs, flat_head, flat_dhead, ldh, rewards, done_u8, T, B, scalars, ws,
                           vs, pg, kw):
  A = dist.param_size
  beh_logits = agent_outputs.policy_logits.to(torch.float32).contiguous()
  actions = agent_outputs.action.contiguous()
  if actions.dtype not in (torch.int32, torch.int64):
    actions = actions.to(torch.int64)
  ops.impala_loss_fwd_bwd(flat_head, ldh, flat_head[A:], ldh, beh_logits, actions, rewards, done_u8, T, B, A,
                          flat_dhead, flat_dhead[A:], scalars, ws, vs, pg, **kw)
  return ()


def _normal_tanh_loss_head(dist, agent, agent_outputs, flat_head, flat_dhead, ldh, rewards, done_u8, T, B, scalars, ws,
                           vs, pg, kw):
  """Continuous actions: float actions [T+1, B, D], behaviour parameters [T+1, B, 2 D], and the standard-normal draws of
  the single-sample entropy estimate, drawn on the device from the distribution's own generator."""
  D, P = dist.num_actions, dist.param_size
  if ldh < P + 1:
    raise ValueError('the agent\'s head row (%d columns) does not hold %d distribution parameters + baseline' % (ldh, P))
  beh = agent_outputs.policy_logits.to(torch.float32).contiguous()
  actions = agent_outputs.action.to(torch.float32).contiguous()
  if tuple(beh.shape) != (T + 1, B, P) or tuple(actions.shape) != (T + 1, B, D):
    raise ValueError('normal_tanh loss: behaviour parameters %s / actions %s, expected %s / %s'
                     % (tuple(beh.shape), tuple(actions.shape), (T + 1, B, P), (T + 1, B, D)))
  noise = dist.draw_noise((T, B, D), flat_head.device, out=agent._buf('entropy_noise', (T, B, D)))
  ops.normal_tanh_loss_fwd_bwd(flat_head, ldh, flat_head[P:], ldh, beh, actions, noise, rewards, done_u8, T, B, D,
                               flat_dhead, flat_dhead[P:], scalars, ws, vs, pg, **kw)
  return (('policy/std', 12),)                        # learner.py:151-152


LOSS_HEADS = {'categorical': _categorical_loss_head, 'normal_tanh': _normal_tanh_loss_head}


def compute_loss(logger, parametric_action_distribution, agent, agent_state, prev_actions, env_outputs,
                 agent_outputs, config=None, mean_denominator=None, want_vtrace=False):
  """learner.py:73-159.  Runs the agent unroll and the fused loss head; the head
  gradient is left in the agent's d_head buffer for `agent.backward()`.

  Returns (total_loss: 0-d device tensor, log_session)."""
  cfg = config or LossConfig()
  logger = logger or DictLogger()
  kw = dict(need_state=False) if getattr(agent, 'accepts_need_state', False) else {}       # the new state is discarded
  learner_outputs, _ = agent(prev_actions, env_outputs, agent_state, unroll=True, is_training=True, **kw)  # :75-79
  head, d_head, ldh = agent.head_buffers()
  T1, B = env_outputs.done.shape[0], env_outputs.done.shape[1]
  T = T1 - 1
  dev = head.device
  rewards = env_outputs.reward.to(torch.float32).contiguous()
  done_u8 = ops.as_u8(env_outputs.done)
  scalars = agent._buf('loss_scalars', (16,))
  ws = agent._buf('loss_ws', (ops.impala_loss_workspace_bytes(T, B) // 4 + 4,))
  vs = agent._buf('vs', (T, B)) if want_vtrace else None
  pg = agent._buf('pg', (T, B)) if want_vtrace else None
  # entropy cost: the agent's own constant, or the learner's learnable parameter (learner.py:121, 127-135, 225-234)
  ecp = agent.entropy_cost_param() if hasattr(agent, 'entropy_cost_param') else None
  own = agent.entropy_cost() if ecp is None else None
  if ecp is not None:
    share = None
    if cfg.target_entropy:
      # data-parallel 'mean': every replica's mean(H) is its SHARE of the global mean, so it takes its share of the target
      share = cfg.target_entropy * float(T * B) / float(mean_denominator or T * B)
    ekw = dict(entropy_cost_param=ecp[0], d_entropy_cost_param=ecp[1], entropy_cost_adjustment_speed=ecp[2],
              target_entropy=share)
  else:
    if cfg.target_entropy:
      raise ValueError('target_entropy needs the learnable entropy cost: construct the agent without its own '
                       'entropy_cost and pass it to a Learner (agents/vtrace/learner.py:225-234)')
    ekw = dict(entropy_cost=float(cfg.entropy_cost if own is None else own))
  ekw.update(baseline_cost=cfg.baseline_cost, kl_cost=cfg.kl_cost, discounting=cfg.discounting, lambda_=cfg.lambda_,
             max_abs_reward=cfg.max_abs_reward, mean_denominator=mean_denominator)
  # the distribution names its fused loss head (the reference's compute_loss is distribution-agnostic, learner.py:95-98)
  kind = getattr(parametric_action_distribution, 'loss_head', 'categorical')
  if kind not in LOSS_HEADS:
    raise NotImplementedError('no fused loss head for a %r distribution (have: %s)' % (kind, ', '.join(sorted(LOSS_HEADS))))
  extra = LOSS_HEADS[kind](parametric_action_distribution, agent, agent_outputs, head.view(-1), d_head.view(-1), ldh,
                           rewards, done_u8, T, B, scalars, ws, vs, pg, ekw)
  session = logger.log_session()
  for name, idx in LOGGED.items():
    logger.log(session, name, scalars[idx])
  logger.log(session, 'policy/entropy_cost', scalars[10])
  for name, idx in extra:
    logger.log(session, name, scalars[idx])
  if want_vtrace:
    session['vtrace/vs'] = vs
    session['vtrace/pg_advantages'] = pg
  return scalars[0], session


def shard_columns(num_columns, rank, world):
  """Contiguous batch-column shard of rank `rank` (every column is an independent
  trajectory; cfg4: 4096 columns -> 8 x 512)."""
  if num_columns % world:
    raise ValueError('batch columns (%d) must divide evenly over %d replicas' % (num_columns, world))
  per = num_columns // world
  return slice(rank * per, (rank + 1) * per)


def all_reduce_gradients(flat_grads, process_group=None, force=False):
  """The one exchange step of a train step: SUM of the flat fp32 gradient bucket over the replicas
  (RCCL over xGMI on GPUs; the reference does this implicitly inside Keras apply_gradients on TPU,
  learner.py:272-275).  With reduction='mean' each replica has already divided its loss by the GLOBAL
  number of (t,b) elements, so the sum equals the single-replica gradient of the global batch; with
  'sum' it reproduces the reference's cross-replica gradient SUM (tests/utils_test.py:609-650)."""
  if torch.distributed.is_available() and torch.distributed.is_initialized() and \
      (force or torch.distributed.get_world_size(process_group) > 1):
    torch.distributed.all_reduce(flat_grads, op=torch.distributed.ReduceOp.SUM, group=process_group)
  return flat_grads


class Learner(object):
  """One data-parallel learner replica: minimize(unroll) = forward + loss + backward +
  gradient all-reduce + Adam (learner.py:255-280)."""

  def __init__(self, agent, optimizer, parametric_action_distribution, config=None,
               reduction='mean', process_group=None, logger=None, force_exchange=False):
    """reduction: 'mean' -> the summed gradient equals a single-replica step at the
    global batch (what matches the reference CPU learner on identical trajectories);
    'sum' -> the reference's multi-replica semantics: per-replica mean losses, gradients
    SUMMED across replicas (tests/utils_test.py:609-650)."""
    assert reduction in ('mean', 'sum')
    self.agent, self.optimizer = agent, optimizer
    self.dist = parametric_action_distribution
    self.config = config or LossConfig()
    self.reduction = reduction
    self.pg = process_group
    self.logger = logger or DictLogger()
    self.world = 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
      self.world = torch.distributed.get_world_size(process_group)
    if force_exchange and not (torch.distributed.is_available() and torch.distributed.is_initialized()):
      raise ValueError('force_exchange needs an initialised process group')
    self.exchanging = self.world > 1 or bool(force_exchange)
    self._pending = []
    # learner.py:225-234: an agent without an entropy_cost of its own gets the learnable one
    if hasattr(agent, 'has_own_entropy_cost') and not agent.has_own_entropy_cost():
      if agent.entropy_cost_param() is None:
        agent.attach_entropy_cost_param(self.config.entropy_cost, self.config.entropy_cost_adjustment_speed)

  def compute_gradients(self, unroll):
    T1, B = unroll.env_outputs.done.shape[0], unroll.env_outputs.done.shape[1]
    n = (T1 - 1) * B * (self.world if self.reduction == 'mean' else 1)
    loss, session = compute_loss(self.logger, self.dist, self.agent, *unroll, config=self.config,
                                 mean_denominator=n)
    self._pending = []
    self.agent.grad_ready_hook = self._on_grads_ready if self.exchanging else None
    try:
      self.agent.backward()
    finally:
      self.agent.grad_ready_hook = None
    return loss, session

  # -- gradient exchange overlapped with the backward pass ------------------------------------------------------ #
  # The agents report ranges of the flat gradient buffer as soon as they are final (`grad_ready_hook(lo, hi)`): for the
  # Atari agents the Dense layer + heads (98 % of the 2.7 MB bucket) are done before the conv backward starts, so
  # their all-reduce flies on RCCL's stream under the remaining ~1 ms of backward kernels and only a ~100 KB
  # exchange of the conv gradients stays exposed.  Ranges that were never reported (agents without hooks, HIP-graph
  # capture) are exchanged in reduce_gradients(): the result is always the SUM of the whole bucket.
  def _on_grads_ready(self, lo, hi):
    if not self.exchanging or hi <= lo:
      return
    if self.agent.flat.grads.is_cuda and torch.cuda.is_current_stream_capturing():
      cut = getattr(self, '_capture_cut', None)          # GraphedStep (data parallel): end this graph segment here
      if cut is not None:
        cut(lo, hi)
      return
    work = torch.distributed.all_reduce(self.agent.flat.grads[lo:hi], op=torch.distributed.ReduceOp.SUM,
                                        group=self.pg, async_op=True)
    self._pending.append((lo, hi, work))

  def reduce_gradients(self):
    pending, self._pending = self._pending, []
    n = self.agent.flat.grads.numel()
    for _, _, work in pending:
      work.wait()
    if not self.exchanging:
      return
    covered, pos = sorted((lo, hi) for lo, hi, _ in pending), 0
    for lo, hi in covered + [(n, n)]:
      if lo < pos:
        raise RuntimeError('overlapping gradient ranges reported by the agent: [%d, %d) after %d' % (lo, hi, pos))
      if lo > pos:
        all_reduce_gradients(self.agent.flat.grads[pos:lo], self.pg, force=True)
      pos = max(pos, hi)
    self.exchange_step_guard()

  def exchange_step_guard(self):
    """The LSTM sequence kernels' sticky abort word travels WITH the gradient exchange (MAX over the replicas): a wait
    that timed out on one rank makes EVERY rank's update kernel drop the step -- the summed gradients contain that rank's
    garbage -- and every rank's host sees the word set one step later, demotes its agent and (GraphedStep) captures its
    graphs again in lock step.  Without it one rank raised while the others blocked in their next all-reduce (ADVICE r4 /
    VERDICT r5 item 8).  Agents without sequence kernels have no guard: no extra collective."""
    guard = getattr(self.agent.flat, 'step_guard', None)
    if guard is not None and self.exchanging:
      torch.distributed.all_reduce(guard, op=torch.distributed.ReduceOp.MAX, group=self.pg)

  def update(self):
    self.optimizer.apply_gradients(self.agent.flat)

  def apply_gradients(self):
    self.reduce_gradients()
    self.update()

  def minimize(self, unroll):
    begin = getattr(self.optimizer, 'begin_step', None)
    if begin is not None and not torch.cuda.is_current_stream_capturing():
      begin(self.agent.flat.params.device)
    loss, session = self.compute_gradients(unroll)
    self.apply_gradients()
    cb = getattr(self.agent, 'end_of_training_step_callback', None)   # learner.py:277-278
    if cb is not None:
      cb()
    return loss, session


class GraphedStep(object):
  """Captures a train step ONCE into HIP graphs and replays it: the ~25 (Atari) to ~600 (R2D2) kernel launches
  of a step become one graph launch, removing the host-side launch gaps (HIP graphs in place of the reference's
  tf.function / XLA step).  Single replica: one graph for the whole step.  Data parallel: compute_gradients is captured
  as a CHAIN of graphs cut where the agent reports a range of the gradient bucket as final (`grad_ready_hook`, at most
  `max_cuts` cuts): after replaying a segment its range's all-reduce is launched asynchronously on RCCL's stream and the
  next segment (the rest of the backward pass) replays under it; whatever was not exchanged by then is exchanged after
  the last segment, then the update graph replays -- the same overlap as the eager path, without its launch gaps.
  The unroll's tensors are the graph's static inputs: copy new trajectories into them (the unroll store can
  write completed unrolls straight into these buffers) and call the object.  Needs an optimizer created with
  capturable=True; everything else on the step is already free of host reads."""

  def __init__(self, learner, unroll, *extra, warmup=2, max_cuts=1):
    if not getattr(learner.optimizer, 'capturable', False):
      raise ValueError('GraphedStep needs optimizers.Adam(..., capturable=True)')
    self.learner, self.unroll, self.extra = learner, unroll, extra
    self._max_cuts = max_cuts
    # The warm-up below runs REAL optimizer steps on whatever the static unroll buffers hold: everything they touch
    # is put back after the capture, so that a graphed learner starts from exactly the state an eager one would
    # (parameters, Adam moments and step counter -- with it the LR-schedule position --, R2D2 target network and
    # target-update phase).
    opt = learner.optimizer
    agents = [a for a in (learner.agent, getattr(learner, 'target_agent', None)) if a is not None]
    saved_params = [a.flat.params.clone() for a in agents]
    sd0 = opt.state_dict()
    saved_opt = dict(iterations=sd0['iterations'], m=None if sd0['m'] is None else sd0['m'].clone(),
                     v=None if sd0['v'] is None else sd0['v'].clone())
    counters = dict((k, getattr(learner, k)) for k in ('iterations',) if hasattr(learner, k))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      for _ in range(warmup):                       # allocates every workspace, loads every code object
        learner.minimize(unroll, *extra)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    opt.begin_step(learner.agent.flat.params.device)
    self.split = bool(getattr(learner, 'exchanging', getattr(learner, 'world', 1) > 1))
    self.graph = torch.cuda.CUDAGraph()
    self.graph2 = None
    if not self.split:
      with torch.cuda.graph(self.graph, capture_error_mode='relaxed'):
        self.outputs = learner.compute_gradients(unroll, *extra)
        learner.update()
    else:
      # segments: [(graph, (lo, hi) | None)] -- the range to exchange asynchronously once that segment has replayed
      self.segments = []
      pool = torch.cuda.graph_pool_handle()
      cap = torch.cuda.Stream()
      state = dict(graph=self.graph, cuts=0)

      def cut(lo, hi):
        if state['cuts'] >= max_cuts or hi <= lo:
          return
        state['cuts'] += 1
        state['graph'].capture_end()
        self.segments.append((state['graph'], (lo, hi)))
        state['graph'] = torch.cuda.CUDAGraph()
        state['graph'].capture_begin(pool=pool, capture_error_mode='relaxed')
      torch.cuda.synchronize()
      cap.wait_stream(torch.cuda.current_stream())
      with torch.cuda.stream(cap):
        self.graph.capture_begin(pool=pool, capture_error_mode='relaxed')
        learner._capture_cut = cut if hasattr(learner, '_on_grads_ready') else None
        ok = False
        try:
          self.outputs = learner.compute_gradients(unroll, *extra)
          ok = True
        finally:
          learner._capture_cut = None
          if ok or torch.cuda.is_current_stream_capturing():
            state['graph'].capture_end()
        self.segments.append((state['graph'], None))
        self.graph2 = torch.cuda.CUDAGraph()
        self.graph2.capture_begin(pool=pool, capture_error_mode='relaxed')
        try:
          learner.update()
        finally:
          self.graph2.capture_end()
      torch.cuda.current_stream().wait_stream(cap)
    # undo the warm-up (in place: the graphs hold these buffers' addresses); the capture itself ran only the Python
    # bookkeeping, not the kernels
    for a, p0 in zip(agents, saved_params):
      a.flat.params.copy_(p0)
    sd = opt.state_dict()
    for k in ('m', 'v'):
      if sd[k] is not None:
        if saved_opt[k] is None:
          sd[k].zero_()
        else:
          sd[k].copy_(saved_opt[k])
    opt.iterations = saved_opt['iterations']
    for k, v in counters.items():
      setattr(learner, k, v)
    self._agents = agents
    # did THIS capture record LSTM sequence kernels?  (with several GraphedSteps over one agent -- one per
    # unroll slot of LearnerServer -- only the first caller sees `_lstm_seq_check()` return True; every graph that still
    # holds the sequence kernels of a demoted agent has to be captured again, so the decision is taken from state)
    self._captured_seq = any(bool(c.get('fused_seq')) for a in agents for c in getattr(a, '_lstm_ctx', {}).values())
    self.exchange = True          # bench.py clears it for a few steps to price the EXPOSED part of the exchange
    torch.cuda.synchronize()

  def __call__(self):
    opt = self.learner.optimizer
    opt.begin_step()
    if not self.split:
      self.graph.replay()
    else:
      lrn = self.learner
      for g, rng in self.segments:
        g.replay()
        if rng is not None and self.exchange:
          lrn._on_grads_ready(*rng)               # asynchronous: flies under the next segment
      if self.exchange:
        lrn.reduce_gradients()                    # waits for those, exchanges the rest
      self.graph2.replay()
    opt.iterations += 1
    post = getattr(self.learner, 'after_graph_replay', None)
    if post is not None:
      post()
    # the persistent LSTM kernels' abort flags: mirrored to pinned host memory after every replay and looked at
    # before the next one (by then the copy has landed: no sync) -- a wait that timed out during a replay raises here
    # Data parallel: the word every rank looks at is the MAX over the ranks (Learner.exchange_step_guard) and the look
    # WAITS for the previous replay's mirror copy -- every rank then takes the decision below at the same step, and the
    # warm-up all-reduces of the new capture meet their partners.  (Single replica: no wait, the mirror is simply looked
    # at once it has landed.)
    for a in self._agents:
      if getattr(a, '_last_lstm', None) is not None:
        a._lstm_seq_check(wait=self.split)        # pylint: disable=protected-access
        a.mirror_error_flags()
    self.recaptured = False
    if self._captured_seq and any(getattr(a, '_seq_demoted', False) for a in self._agents):
      # an agent fell back to the per-step LSTM kernels (a sequence kernel's wait timed out in an earlier replay -- of
      # this graph or of another slot's, on this rank or on another; the update kernel dropped those steps everywhere):
      # this graph still holds the sequence kernels -- capture again.  The step that timed out was dropped ON THE DEVICE;
      # the host-side step counter (Adam's bias correction, the LR schedule position) still advanced for it on every
      # rank alike: a rare fallback, not rolled back.
      out = self.outputs                          # this call's results (the new capture's outputs are not written yet)
      torch.cuda.synchronize()
      self.__init__(self.learner, self.unroll, *self.extra, warmup=1, max_cuts=self._max_cuts)
      self.recaptured = True
      return out
    return self.outputs

  def check_errors(self):
    """Blocking: raises if any replayed step's LSTM sequence kernel aborted."""
    for a in self._agents:
      a.check_errors()
