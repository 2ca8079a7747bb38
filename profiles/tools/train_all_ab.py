"""Developer tool: `train_all.py` three ways in ONE job on one GPU, interleaved, 5 repeats each - what the four environments (ant, halfcheetah, hopper, walker2d) cost per
environment step, after profiles/tools/sweep_ab.py.
  (a) sequential   the four environments (times K seeds) one after another through train(): what four separate jobs do, and the fallback of train_all.py
  (b) per_learner  train_sweep(vary_env=True) with +sweep.schedule=per_learner: the learners in lockstep, one ActingWorker launch and one UpdatePlan.run() per learner per step
  (c) population   train_sweep(vary_env=True) with +sweep.schedule=population: ONE il_act_step_population_mixed launch (two with the exact schedule's append) and ONE
                   mixed-width population update (il_sac_update_population_mixed, il_gail_step_population_mixed) per step
  workload  SAC and GAIL at the shipped shapes (batch 256, actor / critic 256 x 2) on the synthetic stand-ins; one seed (4 learners) and four seeds (16 learners); one
            update per environment step from step 300 on
  rate      aggregate env-steps/s = learners * steps / training_time; training_time is what check_time_usage=true reports (evaluation is off under it)
(c) counts as faster than (b) only if its median beats (b)'s by more than (b)'s spread (max - min) of this job; train_all.py's default schedule becomes `population` only
if that holds at both sizes for both algorithms. The widest learner sets the launch length (ant's layer 1 has K = 128 against 16 or 32): nothing is rebalanced here.
  python profiles/tools/train_all_ab.py [--steps 4000] [--repeats 5] [--seeds 1 4] [--algorithms SAC GAIL] [--out profiles/train_all_ab.txt]"""
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
import train_all
from imitation_learning_amd import config

FORMS = ('sequential', 'per_learner', 'population')
lines = []
out_path = None


def say(text):
  print(text, flush=True)
  lines.append(text)
  if out_path:   # after every line: a job that is cut short keeps the cases it finished
    with open(out_path, 'w') as f: f.write('\n'.join(lines) + '\n')


def overrides(algorithm, steps, start):
  return [f'algorithm={algorithm}', f'steps={steps}', f'training.start={start}', 'training.batch_size=256', 'check_time_usage=true', 'logging.interval=1000',
          '+synthetic_env.dataset_trajectories=6']


def run_form(form, algorithm, K, steps, start, out_dir):
  """The four environments under K seeds (4 K learners) under `form`; returns aggregate env-steps/s."""
  cfgs, prefixes = [], []
  for seed in range(1, K + 1):
    argv = overrides(algorithm, steps, start) + [f'seed={seed}'] + ([] if form == 'sequential' else [f'+sweep.schedule={form}'])
    for c in train_all.env_configs(config.compose(argv), seed):
      cfgs.append(c); prefixes.append(os.path.join(out_dir, str(seed), c.env, ''))
  for p in prefixes: os.makedirs(p, exist_ok=True)
  if form == 'sequential':
    for cfg, p in zip(cfgs, prefixes): train.train(cfg, file_prefix=p)
    torch.cuda.synchronize()
    spent = sum(float(torch.load(p + 'metrics.pth', weights_only=False)['training_time']) for p in prefixes)
  else:
    train.train_sweep(cfgs, prefixes, vary_env=True, noise_ids=[train_all.ENVS.index(c.env) for c in cfgs])
    spent = float(torch.load(prefixes[0] + 'metrics.pth', weights_only=False)['training_time'])   # one clock for the population: every learner reports it
  return len(cfgs) * steps / spent


def report(title, rate):
  med = {k: float(np.median(v)) for k, v in rate.items()}
  say(title)
  for k, v in rate.items():
    say(f'  {k:12s}: median {med[k]:9.0f} env-steps/s  (min {min(v):9.0f} .. max {max(v):9.0f}; repeats ' + ' '.join(f'{r:.0f}' for r in v) + ')')
  spread = max(rate['per_learner']) - min(rate['per_learner'])
  faster = med['population'] - med['per_learner'] > spread
  say(f'  per_learner / sequential = {med["per_learner"] / med["sequential"]:.2f}x, population / sequential = {med["population"] / med["sequential"]:.2f}x, '
      f'population / per_learner = {med["population"] / med["per_learner"]:.2f}x; the per_learner spread is {spread:.0f} env-steps/s: population is '
      f'{"FASTER" if faster else "NOT faster"} than per_learner by more than that')
  return faster


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=4000)
  ap.add_argument('--start', type=int, default=300)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--seeds', type=int, nargs='+', default=[1, 4], help='seeds per case: 4 learners per seed')
  ap.add_argument('--algorithms', nargs='+', default=['SAC', 'GAIL'], choices=['SAC', 'GAIL'])
  ap.add_argument('--out', default=None)
  args = ap.parse_args(argv)
  global out_path
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out_path = os.path.abspath(args.out)
  say(f'device {torch.cuda.get_device_name(0)}; ant, halfcheetah, hopper, walker2d (synthetic stand-ins), batch 256, hidden 256, {args.steps} env steps per learner, one update per step '
      f'from step {args.start}; {args.repeats} interleaved repeats; train.SWEEP_DEFAULT_SCHEDULE = {train.SWEEP_DEFAULT_SCHEDULE}')
  verdicts = []
  with tempfile.TemporaryDirectory() as tmp:
    for algorithm in args.algorithms:
      for K in args.seeds:
        for form in FORMS:   # warm-up: code objects of every launch each form issues
          run_form(form, algorithm, 1, args.start + 100, args.start, os.path.join(tmp, 'warm'))
        rate = {form: [] for form in FORMS}
        for r in range(args.repeats):
          for form in FORMS:   # interleaved: a drift of the machine hits every form alike
            t0 = time.perf_counter()
            rate[form].append(run_form(form, algorithm, K, args.steps, args.start, os.path.join(tmp, f'{algorithm}_{K}_{form}_{r}')))
            print(f'  [{algorithm} {4 * K} learners repeat {r} {form}: {rate[form][-1]:.0f} env-steps/s, {time.perf_counter() - t0:.1f} s wall]', flush=True)
        verdicts.append(report(f'{algorithm}, {K} seed(s) = {4 * K} learners', rate))
  say(f'population faster than per_learner beyond its spread in {sum(verdicts)} of {len(verdicts)} cases -> train_all.py default +sweep.schedule = {"population" if all(verdicts) else "per_learner"}')


if __name__ == '__main__':
  main()
