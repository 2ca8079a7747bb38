"""Developer tool: A/B of PWIL's environment loop (train.py:151-168) and of its expert relabel (train.py:135-141) in ONE job on one GPU, interleaved, 5 repeats each,
every repeat ending in a device synchronise. The baseline is the per-function path of the same job (`+acting.schedule=per_function`, `+pretraining.schedule=per_function`:
`actor(state).sample()`, `compute_reward(...).item()`, `memory.append`, a host-issued `reset()`), against the acting worker with the discriminator as its reward model
(`il_pwil_act_reward` in front of every append) under the exact, fused and overlap schedules, and against `PWILDiscriminator.relabel_memory` (`il_pwil_relabel_rows`).
  size    the timed PWIL size of tests/test_timed_sizes.py: 25,000 atoms, D = 24 (HalfCheetah dims with the absorbing bit), time horizon 1,000; actor / critic 256 x 2
  env     the synthetic HalfCheetah stand-in (host-side, its own rate is printed)
  acting  env-steps/s of the loop alone, and with one PWIL UpdatePlan update (batch 256) per step, issued the way train.py issues it
  relabel rows/s over the first 5,000 rows of the expert memory (an episode end every 1,000 rows)
A worker schedule counts as faster only if its median beats the per-function median by more than the per-function spread (max - min) of this job.
  python profiles/tools/pwil_acting_ab.py [--steps 3000] [--repeats 5] [--rows 5000] [--out profiles/pwil_acting_ab.txt]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import imitation_learning_amd as il
from imitation_learning_amd.environments import make_env

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=3000)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--rows', type=int, default=5000)
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda', 0)
ATOMS, HORIZON, B = 25000, 1000, 256
SCHEDULES = ('per_function', 'exact', 'fused', 'overlap')
lines = []


class Cfg(dict):
  __getattr__ = dict.__getitem__


def say(text):
  print(text, flush=True)
  lines.append(text)


env = make_env('halfcheetah', True)
env.seed(0)
S, A = env.observation_space.shape[0], env.action_space.shape[0]


def expert_memory():
  rs = np.random.RandomState(22)
  states = (rs.standard_normal((ATOMS, S)) * rs.uniform(0.5, 2.0, S) + rs.standard_normal(S)).astype(np.float32)
  states[:, -1] = 0   # the absorbing bit
  timeouts = torch.zeros(ATOMS); timeouts[HORIZON - 1::HORIZON] = 1.0
  t = dict(states=torch.from_numpy(states), actions=torch.from_numpy(rs.uniform(-1, 1, (ATOMS, A)).astype(np.float32)), rewards=torch.zeros(ATOMS), next_states=torch.from_numpy(states),
           terminals=torch.zeros(ATOMS), timeouts=timeouts, weights=torch.ones(ATOMS), num_trajectories=ATOMS // HORIZON)
  return il.ReplayMemory(ATOMS, S, A, True, transitions=t, device=dev)


def discriminator(expert):
  return il.PWILDiscriminator(S, A, Cfg(state_only=False, reward_scale=5, reward_bandwidth_scale=5), expert, HORIZON)


class Learner:
  """What train.py builds for algorithm=PWIL under one acting schedule; `update`: with the UpdatePlan, issued as train.py issues it."""

  def __init__(self, schedule, expert, update):
    torch.manual_seed(0)
    net = Cfg(hidden_size=256, depth=2, activation='relu')
    self.schedule, self.update = schedule, update
    self.actor, self.critic, self.log_alpha = il.SoftActor(S, A, net), il.TwinCritic(S, A, net), torch.zeros(1, device=dev)
    self.memory, self.disc = il.ReplayMemory(100000, S, A, True, device=dev), discriminator(expert)
    self.worker = None if schedule == 'per_function' else il.ActingWorker(self.actor, self.memory, mirror=schedule == 'overlap', reward_model=self.disc)
    self.plan = self.step_update = None
    if update:
      target = il.create_target_network(self.critic)
      opts = il.AdamW(self.actor, lr=3e-4, weight_decay=0), il.AdamW(self.critic, lr=3e-4, weight_decay=0), il.Adam(self.log_alpha, lr=3e-4)
      self.plan = il.UpdatePlan('PWIL', self.actor, self.critic, self.log_alpha, target, self.memory, *opts, B, 0.99, -float(A), 0.995, expert_memory=expert, discriminator=self.disc)
      if schedule == 'overlap': self.worker.attach(self.plan)
      else: self.plan.main_feeds_ring = True

  def prepare_update(self):
    """train.py's first update: eagerly, then recorded as direct launches where that applies, else captured."""
    plan = self.plan
    plan.run()
    if plan.direct_launch_ok():
      plan.record_direct(); self.step_update, self.issue = plan.launch_direct, 'direct launches'
    else:
      plan.capture(warmup=0); self.step_update, self.issue = plan.replay, 'graph replays'
    torch.cuda.synchronize()

  def run(self, steps, update=None):
    """`steps` environment steps of train.py's loop under this schedule; returns env-steps/s."""
    update = self.update if update is None else update
    schedule, worker, memory, actor, disc, plan = self.schedule, self.worker, self.memory, self.actor, self.disc, self.plan
    state, t = env.reset(), 0
    disc.reset()   # a run starts an episode (the previous run's last one was cut short)
    action = worker.act(state) if schedule in ('fused', 'overlap') else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(1, steps + 1):
      if schedule == 'per_function':
        with torch.inference_mode():
          action = actor(state).sample()
          nxt, r, term = env.step(action); t += 1
          memory.append(step, state, action, disc.compute_reward(state, action), nxt, term and t != env.max_episode_steps, t == env.max_episode_steps)
          if term and t != env.max_episode_steps: memory.wrap_for_absorbing_states()
        following = env.reset() if term else nxt
        if term: disc.reset()
      else:
        if schedule == 'exact': action = worker.act(state)
        nxt, r, term = env.step(action); t += 1
        timed_out = t == env.max_episode_steps
        following = env.reset() if term else nxt
        if schedule == 'exact': worker.append(step, nxt, r, term and not timed_out, timed_out)
        elif schedule == 'fused': action = worker.step(step, nxt, r, term and not timed_out, timed_out, obs=following)
        else:
          worker.post(step, state, action, nxt, r, term and not timed_out, timed_out)
          if not update: worker.enqueue_append()   # otherwise the update carries coupling and append
      if term: t = 0
      state = following
      if schedule == 'overlap' and update: worker.act_begin(state)
      if update: self.step_update()
      if schedule == 'overlap': action = worker.act_end() if update else worker.act(state)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def report(title, unit, rate, base):
  med = {k: float(np.median(v)) for k, v in rate.items()}
  spread = max(rate[base]) - min(rate[base])
  say(title)
  for k, v in rate.items():
    say(f'  {k:13s}: median {med[k]:9.0f} {unit}  (min {min(v):9.0f} .. max {max(v):9.0f}; repeats ' + ' '.join(f'{r:.0f}' for r in v) + ')')
  verdict = {}
  for k in rate:
    if k == base: continue
    verdict[k] = med[k] - med[base] > spread
    say(f'  {k} / {base} = {med[k] / med[base]:.2f}x; the {base} spread is {spread:.0f} {unit}: {k} is {"FASTER" if verdict[k] else "NOT faster"} by more than that')
  return med, verdict


say(f'device {torch.cuda.get_device_name(0)}; PWIL against {ATOMS} atoms, D = {S + A}, horizon {HORIZON}; {args.steps} env steps per repeat, {args.repeats} interleaved repeats')
a0, t0 = torch.zeros(1, A), time.perf_counter()
env.reset()
for _ in range(2000): env.step(a0)
say(f'synthetic environment alone: {2000 / (time.perf_counter() - t0):.0f} steps/s')
expert = expert_memory()

for update in (False, True):
  learners = {sch: Learner(sch, expert, update) for sch in SCHEDULES}
  for L in learners.values():
    L.run(400, update=False)   # warm-up: code objects, LDS attributes, and more than one batch of rows in the ring
    if update:
      L.prepare_update(); L.run(200)
  rate = {sch: [] for sch in SCHEDULES}
  for _ in range(args.repeats):
    for sch in SCHEDULES:   # interleaved: a drift of the machine hits every schedule alike
      rate[sch].append(learners[sch].run(args.steps))
  how = ' + one UpdatePlan update per step (' + ', '.join(f'{s}: {L.issue}' for s, L in learners.items()) + ')' if update else ' alone'
  report(f'acting loop{how}', 'env-steps/s', rate, 'per_function')
  bad = [f'{s}: {what}' for s, L in learners.items() for what, t in (('actor', L.actor.flat), ('critic', L.critic.flat), ('ring', L.memory.ring), ('atom weights', L.disc.expert_weights)) if not torch.isfinite(t).all()]
  assert not bad, 'non-finite values after the timed runs: ' + ', '.join(bad)
  del learners

rows = min(args.rows, ATOMS)
d_loop, d_dev = discriminator(expert), discriminator(expert)


def row_loop():
  for i in range(rows):
    tr = expert[i]
    expert.rewards[i] = d_loop.compute_reward(tr['states'].unsqueeze(0), tr['actions'].unsqueeze(0))
    if tr['terminals'] or tr['timeouts']: d_loop.reset()


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return time.perf_counter() - t0


rate = dict(row_loop=[], relabel_memory=[])
d_dev.relabel_memory(expert, 0, 64)
d_dev.reset()
for _ in range(args.repeats):
  d_loop.reset(); rate['row_loop'].append(rows / timed(row_loop))
  by_loop = expert.rewards[:rows].clone()
  d_dev.reset(); rate['relabel_memory'].append(rows / timed(lambda: d_dev.relabel_memory(expert, 0, rows)))
  assert torch.equal(by_loop, expert.rewards[:rows]) and torch.equal(d_loop.expert_weights, d_dev.expert_weights), 'relabel_memory and the row loop disagree'
report(f'expert relabel over {rows} rows (bit-identical rewards and weights, checked every repeat)', 'rows/s', rate, 'row_loop')

if args.out:
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f: f.write('\n'.join(lines) + '\n')
