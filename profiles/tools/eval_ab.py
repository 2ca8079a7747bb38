"""Developer tool: what one evaluation costs under `+evaluation.schedule=sequential` and under `lockstep`, on one GPU in ONE job, 5 interleaved repeats each.
  agent       evaluate_agent (one environment, the episodes one after another: a get_greedy_action turn-around per episode step) against evaluate_agent_lockstep
              (one seeded environment per episode, ONE il_act_eval_rows launch per lockstep step) at 30 episodes, horizon 1,000, HalfCheetah dims, hidden 256
  population  evaluate_population (the L learners in lockstep, each learner's episodes one after another: one il_act_step_population launch per step) against
              evaluate_population_lockstep (one launch per lockstep step for all L x 30 rows) at L = 4 and 16
  train       the share of wall time a 20,000-step `train.py algorithm=SAC env=halfcheetah` run spends in evaluation (evaluation.interval=10000, evaluation.episodes=30:
              two evaluations), under each schedule
Reported: median seconds per evaluation and the spread (max - min) over the repeats. The sequential timings are the baseline - that code is untouched -; lockstep counts as
faster only where its median beats the sequential median by more than the sequential spread of this job. The parts are separate commands so that each runs under a time
limit of its own, chained so that the first failure ends the job; every part appends to the same file:
  timeout -k 10 300 python profiles/tools/eval_ab.py --part agent --out profiles/eval_ab.txt --fresh && \\
  timeout -k 10 420 python profiles/tools/eval_ab.py --part population --out profiles/eval_ab.txt && \\
  timeout -k 10 300 python profiles/tools/eval_ab.py --part train --out profiles/eval_ab.txt
`--actor DEPTH ACTIVATION HIDDEN` (part agent) times another actor shape - a general one goes through il.GeneralLockstepEvaluator (ONE il_act_eval_rows_general launch per
lockstep step) against the same untouched sequential code; without it the shape is the default's and the three commands above reproduce the file as it was:
  timeout -k 10 300 python profiles/tools/eval_ab.py --part agent --actor 3 tanh 256 --out profiles/eval_ab.txt && \\
  timeout -k 10 420 python profiles/tools/eval_ab.py --part agent --actor 8 tanh 512 --out profiles/eval_ab.txt"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import train
import imitation_learning_amd as il
from imitation_learning_amd import config
from imitation_learning_amd.environments import SyntheticD4RLEnv, env_dims
from imitation_learning_amd.evaluation import evaluate_agent, evaluate_population

ENV, HIDDEN = 'halfcheetah', 256
out_path = None


def say(text):
  print(text, flush=True)
  if out_path:   # after every line: a job that is cut short keeps what it finished
    with open(out_path, 'a') as f: f.write(text + '\n')


ACTOR = []   # --actor: overrides of reinforcement.actor (empty: the default shape)


def actor_of(seed):
  S, A = env_dims(ENV, True)
  torch.manual_seed(seed)
  return il.SoftActor(S, A, config.compose(['algorithm=SAC'] + ACTOR).reinforcement.actor)


def envs_of(seed, copies, horizon):
  out = []
  for k in range(copies):
    env = SyntheticD4RLEnv(ENV, True, max_episode_steps=horizon)
    env.seed(config.eval_env_seed(seed, k))
    out.append(env)
  return out


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return time.perf_counter() - t0


def report(title, secs):
  med = {k: float(np.median(v)) for k, v in secs.items()}
  say(title)
  for k, v in secs.items():
    say(f'  {k:10s}: median {med[k]:7.3f} s per evaluation  (min {min(v):7.3f} .. max {max(v):7.3f}; repeats ' + ' '.join(f'{r:.3f}' for r in v) + ')')
  spread = max(secs['sequential']) - min(secs['sequential'])
  faster = med['sequential'] - med['lockstep'] > spread
  say(f'  sequential / lockstep = {med["sequential"] / med["lockstep"]:.2f}x; the sequential spread is {spread:.3f} s: lockstep is {"FASTER" if faster else "NOT faster"} than sequential by more than that')


def part_agent(args):
  actor, E, T = actor_of(1), args.episodes, args.horizon
  seq_env, lock_envs = envs_of(1, 1, T)[0], envs_of(1, E, T)
  evaluator = (il.GeneralLockstepEvaluator if actor.general else il.LockstepEvaluator)([actor], E)
  forms = dict(sequential=lambda: evaluate_agent(actor, seq_env, E), lockstep=lambda: il.evaluate_agent_lockstep(actor, lock_envs, E, evaluator=evaluator))
  for fn in forms.values(): fn()   # warm-up: code objects, allocator
  secs = {k: [] for k in forms}
  for _ in range(args.repeats):
    for k, fn in forms.items(): secs[k].append(timed(fn))   # interleaved: a drift of the machine hits both alike
  shape = f' [actor depth {actor.depth} / {actor.activation} / hidden {actor.hidden}: {type(evaluator).__name__}]' if ACTOR else ''
  report(f'one learner: evaluate_agent against evaluate_agent_lockstep, {E} episodes, horizon {T} ({E * T} greedy steps){shape}', secs)


def part_population(args):
  E, T = args.episodes, args.horizon
  S, A = env_dims(ENV, True)
  for L in args.learners:
    actors = [actor_of(1 + l) for l in range(L)]
    memories = [il.ReplayMemory(64, S, A, True) for _ in range(L)]
    worker = il.PopulationActingWorker(actors, memories, list(range(1, L + 1)))
    evaluator = il.LockstepEvaluator(actors, E)
    seq_envs, lock_envs = [envs_of(1 + l, 1, T)[0] for l in range(L)], [envs_of(1 + l, E, T) for l in range(L)]
    forms = dict(sequential=lambda: evaluate_population(worker, seq_envs, E), lockstep=lambda: il.evaluate_population_lockstep(evaluator, lock_envs, E))
    for fn in forms.values(): fn()
    secs = {k: [] for k in forms}
    for _ in range(args.repeats):
      for k, fn in forms.items(): secs[k].append(timed(fn))
    report(f'{L} learners: evaluate_population against evaluate_population_lockstep, {E} episodes each, horizon {T} ({L * E * T} greedy steps)', secs)


def part_train(args):
  spent = [0.0]

  def clocked(fn):
    def wrapper(*a, **k):
      t0 = time.perf_counter()
      try: return fn(*a, **k)
      finally: spent[0] += time.perf_counter() - t0
    return wrapper
  train.evaluate_agent, train.evaluate_agent_lockstep = clocked(train.evaluate_agent), clocked(train.evaluate_agent_lockstep)
  base = ['algorithm=SAC', f'env={ENV}', f'steps={args.train_steps}', 'seed=1', '+synthetic_env.dataset_trajectories=6']
  say(f'train.py {" ".join(base)} (evaluation.interval=10000, evaluation.episodes=30, horizon 1000): wall time and the share of it spent in evaluation')
  with tempfile.TemporaryDirectory() as tmp:
    for r in range(args.train_repeats):
      for schedule in config.EVALUATION_SCHEDULES:
        d = os.path.join(tmp, f'{schedule}_{r}')
        os.makedirs(d)
        os.chdir(d)
        spent[0] = 0.0
        wall = timed(lambda: train.train(config.compose(base + [f'+evaluation.schedule={schedule}'])))
        say(f'  {schedule:10s} run {r}: {wall:7.2f} s wall, {spent[0]:7.2f} s in evaluation = {100 * spent[0] / wall:5.1f} %')
        os.chdir(ROOT)


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--part', required=True, choices=['agent', 'population', 'train'])
  ap.add_argument('--episodes', type=int, default=30)
  ap.add_argument('--horizon', type=int, default=1000)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--learners', type=int, nargs='+', default=[4, 16])
  ap.add_argument('--train-steps', type=int, default=20000)
  ap.add_argument('--train-repeats', type=int, default=2)
  ap.add_argument('--actor', nargs=3, metavar=('DEPTH', 'ACTIVATION', 'HIDDEN'), default=None, help='part agent: the actor shape (default: that of the configuration, depth 2 / relu / 256)')
  ap.add_argument('--out', default=None)
  ap.add_argument('--fresh', action='store_true', help='start the output file anew (the first part of a job)')
  args = ap.parse_args(argv)
  global out_path
  if args.actor:
    assert args.part == 'agent', '--actor: part agent only'
    ACTOR[:] = [f'reinforcement.actor.depth={int(args.actor[0])}', f'reinforcement.actor.activation={args.actor[1]}', f'reinforcement.actor.hidden_size={int(args.actor[2])}']
  if args.out:
    out_path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    if args.fresh and os.path.exists(out_path): os.remove(out_path)
  if args.fresh or not args.out:
    say(f'device {torch.cuda.get_device_name(0)}; {ENV} dims (synthetic stand-in, absorbing bit on), actor 256 x 2; {args.repeats} interleaved repeats per case; '
        f'config.EVALUATION_DEFAULT_SCHEDULE = {config.EVALUATION_DEFAULT_SCHEDULE}')
  dict(agent=part_agent, population=part_population, train=part_train)[args.part](args)


if __name__ == '__main__':
  main()
