"""Env-steps/s of the acting path on the synthetic HalfCheetah stand-in: per-function calls vs il_act_step
(exact / overlap schedules), without updates and with one captured GAIL update per env step.  Usage: python profiles/tools/acting_bench.py

General actor shapes (il_act_step_general): `--actor-depth D --actor-activation relu|tanh|sigmoid --actor-hidden H [--env NAME] [--repeats 5] [--steps 3000] [--out FILE]`
times the acting loop alone (no updates: the yardstick is the per-function path of the same job) - `--repeats` INTERLEAVED repeats of per_function / exact / fused /
overlap, env-steps/s each and the act turn-around (post -> echo of one `worker.act`, or `actor(state).sample()` + the copy to the host), plus the fused shape's
turn-around in the same job for scale. Several shapes in one job: repeat the three options' values comma-separated (`--actor-depth 3,8 --actor-hidden 256,512 ...`)."""
import argparse
import json
import statistics
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
import bench  # noqa: E402
import imitation_learning_amd as il  # noqa: E402
from imitation_learning_amd.environments import make_env  # noqa: E402


def loop(schedule, plan, actor, memory, env, steps, update, early_act=True, direct=True, thread=False):
  worker = il.ActingWorker(actor, memory, mirror=schedule == 'overlap') if schedule != 'per_function' else None
  step_update = plan.replay if plan is not None else None   # (plan = None: the acting loop alone)
  if schedule == 'overlap' and update:   # the update with this worker's append before and its snapshot after: recorded as direct launches (round 6), or re-captured as graphs
    plan.graph = plan.graph_side = None; plan.pre_hooks.clear(); plan.post_hooks.clear()
    worker.attach(plan)
    if direct and plan.direct_launch_ok():
      plan.record_direct(); step_update = plan.launch_async if thread else plan.launch_direct
    else:
      plan.capture(warmup=0)
  state, t = env.reset(), 0
  action = worker.act(state) if schedule in ('fused', 'overlap') else None
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for step in range(1, steps + 1):
    if worker is None:
      action = actor(state).sample()
      nxt, r, term = env.step(action); t += 1
      memory.append(step, state, action, r, nxt, term and t != env.max_episode_steps, t == env.max_episode_steps)
      if term and t != env.max_episode_steps: memory.wrap_for_absorbing_states()
      state = env.reset() if term else nxt
    elif schedule == 'exact':
      action = worker.act(state)
      nxt, r, term = env.step(action); t += 1
      worker.append(step, nxt, r, term and t != env.max_episode_steps, t == env.max_episode_steps)
      state = env.reset() if term else nxt
    elif schedule == 'fused':
      nxt, r, term = env.step(action); t += 1
      action = worker.step(step, nxt, r, term and t != env.max_episode_steps, t == env.max_episode_steps, obs=env.reset() if term else None)
    else:
      nxt, r, term = env.step(action); t += 1
      worker.post(step, state, action, nxt, r, term and t != env.max_episode_steps, t == env.max_episode_steps)
      state = env.reset() if term else nxt
      if not update: worker.enqueue_append()
    if term: t = 0
    if schedule == 'overlap' and early_act: worker.act_begin(state)   # (round 6) the act launch ahead of the update's host work: its turn-around hides behind the replay
    if update: step_update()
    if schedule == 'overlap': action = worker.act_end() if early_act else worker.act(state)
  if plan is not None: plan.launcher_wait()
  torch.cuda.synchronize()
  return steps / (time.perf_counter() - t0)


def turnaround_us(schedule, actor, memory, env, n=2000):
  """Median microseconds from posting an observation to holding its action on the host."""
  worker = il.ActingWorker(actor, memory, mirror=schedule == 'overlap') if schedule != 'per_function' else None
  state, times = env.reset(), []
  for i in range(n + 200):
    t0 = time.perf_counter()
    a = worker.act(state) if worker is not None else actor(state).sample().cpu()
    if i >= 200: times.append(time.perf_counter() - t0)
  torch.cuda.synchronize()
  return round(statistics.median(times) * 1e6, 2)


def general(args):
  """Acting loop alone for general actor shapes: interleaved repeats of every schedule the shape supports."""
  dev = torch.device('cuda', 0)

  class Cfg(dict):
    __getattr__ = dict.__getitem__
  env = make_env(args.env, True)
  env.seed(0)
  S, A = env.observation_space.shape[0], env.action_space.shape[0]
  out = dict(env=args.env, state_size=S, action_size=A, repeats=args.repeats, steps_per_repeat=args.steps, note='acting loop alone, no updates; env-steps/s; turn-around = median us of one act')
  s0, t0 = env.reset(), time.perf_counter()
  for _ in range(2000): env.step(torch.zeros(1, A))
  out['env_only_steps_per_s'] = round(2000 / (time.perf_counter() - t0), 1)
  fused_actor = il.SoftActor(S, A, Cfg(hidden_size=256, depth=2, activation='relu'), device=dev)
  out['fused_shape_turnaround_us'] = {sch: turnaround_us(sch, fused_actor, il.ReplayMemory(100000, S, A, True, device=dev), env) for sch in ('per_function', 'exact', 'overlap')}
  shapes = list(zip(args.actor_depth.split(','), args.actor_activation.split(','), args.actor_hidden.split(',')))
  out['shapes'] = {}
  for depth, activation, hidden in shapes:
    actor = il.SoftActor(S, A, Cfg(hidden_size=int(hidden), depth=int(depth), activation=activation), device=dev)
    memory = il.ReplayMemory(100000, S, A, True, device=dev)
    one_launch = il.ActingWorker(actor, memory).one_launch
    schedules = ('per_function', 'exact', 'fused') + (('overlap',) if one_launch else ())
    for sch in schedules: loop(sch, None, actor, memory, env, 300, False)   # warm-up: code objects, LDS attributes
    rates = {sch: [] for sch in schedules}
    for _ in range(args.repeats):
      for sch in schedules:   # interleaved: a drift of the box hits every schedule alike
        rates[sch].append(round(loop(sch, None, actor, memory, env, args.steps, False), 1))
    res = dict(one_launch=bool(one_launch), parameters_MB=round(actor.flat.numel() * 4 / 1e6, 3))
    for sch in schedules:
      r = rates[sch]
      res[sch] = dict(env_steps_per_s=r, median=statistics.median(r), min=min(r), max=max(r), turnaround_us=turnaround_us(sch, actor, memory, env) if sch != 'fused' else None)
    out['shapes'][f'depth{depth}_{activation}_h{hidden}'] = res
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f: f.write(text + '\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--actor-depth', default=None); ap.add_argument('--actor-activation', default='relu'); ap.add_argument('--actor-hidden', default='256')
  ap.add_argument('--env', default='halfcheetah'); ap.add_argument('--repeats', type=int, default=5); ap.add_argument('--steps', type=int, default=3000); ap.add_argument('--out', default=None)
  args = ap.parse_args()
  if args.actor_depth is not None:
    return general(args)
  dev = torch.device('cuda', 0)
  plan, nets, _ = bench.build(dev, 0)
  actor, memory = nets[0], plan.memory
  env = make_env('halfcheetah', True)
  env.seed(0)
  for _ in range(3): plan.run()
  plan.capture(warmup=0)
  # host-only cost of the environment itself, for reference
  s, t0 = env.reset(), time.perf_counter()
  a = torch.zeros(1, 6)
  for _ in range(2000): env.step(a)
  env_only = 2000 / (time.perf_counter() - t0)
  out = dict(env_only_steps_per_s=round(env_only, 1))
  for update in (False, True):
    for schedule in ('per_function', 'exact', 'fused', 'overlap'):
      loop(schedule, plan, actor, memory, env, 200, update)
      out[f'{schedule}{"+update" if update else ""}'] = round(loop(schedule, plan, actor, memory, env, 3000, update), 1)
  loop('overlap', plan, actor, memory, env, 200, True, thread=True)
  out['overlap+update (launcher thread: UpdatePlan.launch_async)'] = round(loop('overlap', plan, actor, memory, env, 3000, True, thread=True), 1)
  loop('overlap', plan, actor, memory, env, 200, True, direct=False)
  out['overlap+update (graph replays instead of direct launches)'] = round(loop('overlap', plan, actor, memory, env, 3000, True, direct=False), 1)
  loop('overlap', plan, actor, memory, env, 200, True, early_act=False, direct=False)
  out['overlap+update (graph replays, act launched behind the replay: round 5)'] = round(loop('overlap', plan, actor, memory, env, 3000, True, early_act=False, direct=False), 1)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
