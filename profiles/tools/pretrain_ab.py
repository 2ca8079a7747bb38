"""Developer tool: A/B of the expert-data pretraining loops (train.py:93-123) - the per-function loop (`train.expert_batches` + one update call per iteration, what
`+pretraining.schedule=per_function` runs) against the device-resident epoch (`il.PretrainPlan`, the default) - in ONE job, interleaved, 5 repeats each, every repeat
ending in a device synchronise. Three shapes:
  BC    BASELINE.json configs[0]: hopper dims, hidden 256, batch 256, 5,000 expert rows (bc_pretraining: lr 2.5e-4)
  DRIL  conf/algorithm/DRIL.yaml's discriminator: hidden 64, depth 1, tanh, input_dropout 0.1, dropout 0.1 (lr 3e-5)
  RED   conf/algorithm/RED.yaml's: hidden 32, depth 1, relu, no dropout (lr 3e-5)
Prints iterations/s (median and min .. max over the repeats) per schedule and shape, and whether the plan's median is below the loop's by more than the loop's own
spread in this job.
  python profiles/tools/pretrain_ab.py [--iterations 1000] [--repeats 5] > profiles/pretrain_ab.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import imitation_learning_amd as il
import train

ap = argparse.ArgumentParser()
ap.add_argument('--iterations', type=int, default=1000)
ap.add_argument('--repeats', type=int, default=5)
args = ap.parse_args()
dev = torch.device('cuda', 0)
S, A, B, ROWS = 12, 3, 256, 5000


class Cfg(dict):
  __getattr__ = dict.__getitem__


def expert_memory():
  rs = np.random.RandomState(100)
  z = torch.zeros(ROWS)
  states = torch.from_numpy((rs.standard_normal((ROWS, S)) + 0.5).astype(np.float32))
  t = dict(states=states, actions=torch.from_numpy(rs.uniform(-1, 1, (ROWS, A)).astype(np.float32)), rewards=z, next_states=states, terminals=z, timeouts=z,
           weights=torch.ones(ROWS), num_trajectories=5)
  return il.ReplayMemory(ROWS, S, A, False, transitions=t, device=dev)


def models(kind):
  torch.manual_seed(0)
  if kind == 'BC':
    m = il.SoftActor(S, A, Cfg(hidden_size=256, depth=2, activation='relu'))
    return m, il.AdamW(m, lr=2.5e-4, weight_decay=0)
  if kind == 'DRIL':
    m = il.SoftActor(S, A, Cfg(hidden_size=64, depth=1, activation='tanh', input_dropout=0.1, dropout=0.1))
  else:
    m = il.REDDiscriminator(S, A, Cfg(state_only=False, reward_bandwidth_scale=0, discriminator=Cfg(hidden_size=32, depth=1, activation='relu', input_dropout=0, dropout=0)))
  return m, il.AdamW(m, lr=3e-5, weight_decay=0)


def loop(kind, model, opt, mem, cfg, count):
  """train.py's own loop (the per_function schedule)."""
  for batch in train.expert_batches(cfg, mem, S, A, count):
    if kind == 'RED': il.target_estimation_update(model, batch, opt)
    else: il.behavioural_cloning_update(model, batch, opt)


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return time.perf_counter() - t0


mem = expert_memory()
cfg = Cfg(seed=0, training=Cfg(batch_size=B), imitation=Cfg(absorbing=False))
print(f'device {torch.cuda.get_device_name(0)}; {args.iterations} iterations per repeat, {args.repeats} interleaved repeats, batch {B}, {ROWS} expert rows', flush=True)
slower = []
for kind in ('BC', 'DRIL', 'RED'):
  (ml, ol), (mp, op) = models(kind), models(kind)
  plan = il.PretrainPlan(kind, mp, op, mem, B, torch.Generator().manual_seed(0))
  timed(lambda: loop(kind, ml, ol, mem, cfg, 100)); timed(lambda: plan.run(100))   # warm-up: code objects, workspaces, the first table half
  rate = dict(loop=[], plan=[])
  for _ in range(args.repeats):
    rate['loop'].append(args.iterations / timed(lambda: loop(kind, ml, ol, mem, cfg, args.iterations)))
    rate['plan'].append(args.iterations / timed(lambda: plan.run(args.iterations)))
  med = {k: float(np.median(v)) for k, v in rate.items()}
  spread = max(rate['loop']) - min(rate['loop'])
  for k in ('loop', 'plan'):
    print(f'{kind:4s} {k:4s}: median {med[k]:9.0f} iterations/s  (min {min(rate[k]):9.0f} .. max {max(rate[k]):9.0f}; repeats ' + ' '.join(f'{r:.0f}' for r in rate[k]) + ')', flush=True)
  ok = med['plan'] >= med['loop'] - spread
  if not ok: slower.append(kind)
  print(f'{kind:4s} plan / loop = {med["plan"] / med["loop"]:.2f}x; the loop\'s spread is {spread:.0f} iterations/s: the plan is {"NOT below" if ok else "BELOW"} the loop by more than that', flush=True)
  assert all(torch.isfinite(t).all() for t in (mp.flat, ml.flat))
print('speed criterion: ' + ('met for all three shapes' if not slower else 'MISSED for ' + ', '.join(slower)), flush=True)
