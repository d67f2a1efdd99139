"""Times the fused V-trace loss heads at learner sizes: the tanh-Gaussian head (csrc/loss_normal_tanh.hip) and the
categorical head at the same row width (A = 2 D), T = 20, B = 512, D in {6, 17}.  Every shape is warmed up first; the two
heads are timed alternately (several rounds of `--iters` back-to-back launches between device events), and the median
round is reported.  Prints one JSON line; needs a GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seed_rl_amd import ops  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=2000)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=200)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_normal_tanh_loss needs a GPU')
  dev = torch.device('cuda:0')
  T, B = 20, 512
  rng = np.random.default_rng(0)
  t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  result = dict(T=T, B=B, iters=args.iters, rounds=args.rounds, device=torch.cuda.get_device_name(0), shapes=[])
  for D in (6, 17):
    A, T1 = 2 * D, T + 1
    ld = (A + 1 + 3) // 4 * 4
    head = t(rng.uniform(-1, 1, (T1, B, ld)).astype(np.float32)).view(-1)
    d_head = torch.zeros_like(head)
    beh = t(rng.uniform(-1, 1, (T1, B, A)).astype(np.float32))
    act_f = t(np.tanh(rng.standard_normal((T1, B, D))).astype(np.float32))
    act_i = t(rng.integers(0, A, (T1, B)).astype(np.int64))
    noise = t(rng.standard_normal((T, B, D)).astype(np.float32))
    rew = t(rng.standard_normal((T1, B)).astype(np.float32))
    done = ops.as_u8(t(rng.uniform(size=(T1, B)) < 0.1))
    scalars = torch.zeros(16, device=dev)
    ws = torch.zeros(ops.impala_loss_workspace_bytes(T, B) // 4 + 4, device=dev)
    heads = dict(
        normal_tanh=lambda: ops.normal_tanh_loss_fwd_bwd(head, ld, head[A:], ld, beh, act_f, noise, rew, done, T, B, D,
                                                         d_head, d_head[A:], scalars, ws),
        categorical=lambda: ops.impala_loss_fwd_bwd(head, ld, head[A:], ld, beh, act_i, rew, done, T, B, A, d_head,
                                                    d_head[A:], scalars, ws))
    times = dict((k, []) for k in heads)
    for fn in heads.values():
      for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
      for name, fn in heads.items():                  # alternate the two heads within a round
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
          fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
    med = dict((k, float(np.median(v))) for k, v in times.items())
    result['shapes'].append(dict(D=D, A=A, normal_tanh_us=med['normal_tanh'], categorical_us=med['categorical'],
                                 ratio=med['normal_tanh'] / med['categorical'],
                                 normal_tanh_us_min_max=[min(times['normal_tanh']), max(times['normal_tanh'])],
                                 categorical_us_min_max=[min(times['categorical']), max(times['categorical'])]))
  print(json.dumps(result))


if __name__ == '__main__':
  main()
