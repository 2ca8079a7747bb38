"""Developer tool: a seed sweep three ways in ONE job on one GPU, interleaved, 5 repeats each - what `python train.py -m seed=...` costs per environment step.
  (a) sequential   the L jobs one after another through train() (what Hydra's basic launcher does, and all that was possible before the sweep driver): the baseline
  (b) per_learner  train_sweep with +sweep.schedule=per_learner: L learners in lockstep, one ActingWorker launch and one UpdatePlan.run() per learner per step
  (c) population   train_sweep with +sweep.schedule=population: ONE il_act_step_population launch (two with the exact schedule's append) and ONE population update per step
  workload  GAIL and SAC on halfcheetah (the synthetic stand-in), batch 256, actor / critic 256 x 2, L = 4 and 16, one update per environment step from step 300 on
  rate      aggregate env-steps/s = L * steps / training_time; training_time is what check_time_usage=true reports (everything behind the construction of environments,
            expert data and networks: plan set-up, the loop, every launch drained before the clock stops; evaluation is off under check_time_usage)
(c) counts as faster than (b) only if its median beats (b)'s by more than (b)'s spread (max - min) of this job; the default of +sweep.schedule follows from that at both L.
  python profiles/tools/sweep_ab.py [--steps 4000] [--repeats 5] [--learners 4 16] [--algorithms GAIL SAC] [--out profiles/sweep_ab.txt]
(--algorithms RED: the same three forms with the predictor's pretraining cut to 100 iterations per learner; --algorithms GMMIL: at batch 128, the batch of every shipped GMMIL
configuration, where one reward launch is 16 workgroups; --algorithms DRIL: the shipped configuration, i.e. with imitation.bc_aux_loss - il_dril_reward_population and
il_bc_step_population per update - and the ensemble's pretraining cut to 100 iterations per learner; --algorithms PWIL: with the opt-in key +sweep.pwil_population=true,
every learner on its own 6,006 atoms - six trajectories of 1,000 steps and their absorbing rows - at horizon 1,000: 24 chunks of 8 candidates per learner, one
il_pwil_act_reward_population launch per lockstep step under (c) against one il_pwil_act_reward launch per learner under (b); (a) couples per step as train() does;
--algorithms AdRIL: the shipped configuration - balanced, update_freq 1250 - with the opt-in key +sweep.adril_population=true: one il_batch_mix_relabel_population launch
and one copy of 3 L words per update under (c) against one il_batch_mix_relabel_dyn launch and one three-word copy per learner under (b); --algorithms GAIL_Mixup: GAIL with
imitation.loss_function=Mixup at the default mixup_alpha = 1 and the opt-in key +sweep.gail_mixup_population=true - il_gail_mixup_step_population per update under (c) against
il_gail_disc_step + il_gail_reward per learner under (b); GAIL_Mixup_0.5: the same at imitation.mixup_alpha=0.5, one coefficient launch for all learners under (c))"""
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
  extra = ['imitation.pretraining.iterations=100'] if algorithm in ('RED', 'DRIL') else []   # (the predictor's / ensemble's pretraining sits in front of the clock: kept short, the job measures the loop)
  if algorithm == 'PWIL': extra = [train.PWIL_POPULATION_KEY]   # PWIL sweeps form a population on opt-in only; train() ignores the key
  if algorithm == 'AdRIL': extra = [train.ADRIL_POPULATION_KEY]   # likewise
  if algorithm.startswith('GAIL_Mixup'):   # GAIL whose loss is Mixup, under its opt-in key; GAIL_Mixup_<alpha>: at that mixup_alpha
    extra = ['imitation.loss_function=Mixup', train.GAIL_MIXUP_POPULATION_KEY] + ([f'imitation.mixup_alpha={algorithm.split("_")[2]}'] if algorithm.count('_') == 2 else [])
    algorithm = 'GAIL'
  batch = 128 if algorithm == 'GMMIL' else 256
  return [f'algorithm={algorithm}', 'env=halfcheetah', f'steps={steps}', f'training.start={start}', f'training.batch_size={batch}', 'check_time_usage=true', 'logging.interval=1000',
          '+synthetic_env.dataset_trajectories=6'] + extra


def run_form(form, algorithm, L, steps, start, out_dir):
  """One sweep of L seeds under `form`; returns aggregate env-steps/s over the summed training_time of its jobs."""
  os.makedirs(out_dir, exist_ok=True)
  seeds = ','.join(str(s) for s in range(1, L + 1))
  argv = ['-m', f'seed={seeds}'] + overrides(algorithm, steps, start)
  prefixes = [os.path.join(out_dir, str(j), '') for j in range(L)]
  for p in prefixes: os.makedirs(p, exist_ok=True)
  if form == 'sequential':
    cfgs, _ = config.compose_multirun(argv)
    for cfg, p in zip(cfgs, prefixes): train.train(cfg, file_prefix=p)
    torch.cuda.synchronize()
    spent = sum(float(torch.load(p + 'metrics.pth', weights_only=False)['training_time']) for p in prefixes)
  else:
    cfgs, _ = config.compose_multirun(argv + [f'+sweep.schedule={form}'])
    train.train_sweep(cfgs, prefixes)
    spent = float(torch.load(prefixes[0] + 'metrics.pth', weights_only=False)['training_time'])   # one clock for the population: every job reports it
  return L * steps / spent


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
  ap.add_argument('--learners', type=int, nargs='+', default=[4, 16])
  ap.add_argument('--algorithms', nargs='+', default=['GAIL', 'SAC'], choices=['GAIL', 'SAC', 'RED', 'GMMIL', 'DRIL', 'PWIL', 'AdRIL', 'GAIL_Mixup', 'GAIL_Mixup_0.5'])
  ap.add_argument('--out', default=None)
  args = ap.parse_args(argv)
  global out_path
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out_path = os.path.abspath(args.out)
  say(f'device {torch.cuda.get_device_name(0)}; halfcheetah (synthetic stand-in), batch 256 (GMMIL: 128), {args.steps} env steps per learner, one update per step from step {args.start}; '
      f'{args.repeats} interleaved repeats; train.SWEEP_DEFAULT_SCHEDULE = {train.SWEEP_DEFAULT_SCHEDULE}')
  verdicts = []
  with tempfile.TemporaryDirectory() as tmp:
    for algorithm in args.algorithms:
      for L in args.learners:
        for form in FORMS:   # warm-up: code objects of every launch each form issues
          run_form(form, algorithm, min(L, 2), args.start + 100, args.start, os.path.join(tmp, 'warm'))
        rate = {form: [] for form in FORMS}
        for r in range(args.repeats):
          for form in FORMS:   # interleaved: a drift of the machine hits every form alike
            t0 = time.perf_counter()
            rate[form].append(run_form(form, algorithm, L, args.steps, args.start, os.path.join(tmp, f'{algorithm}_{L}_{form}_{r}')))
            print(f'  [{algorithm} L={L} repeat {r} {form}: {rate[form][-1]:.0f} env-steps/s, {time.perf_counter() - t0:.1f} s wall]', flush=True)
        verdicts.append(report(f'{algorithm}, L = {L} learners', rate))
  say(f'population faster than per_learner beyond its spread in {sum(verdicts)} of {len(verdicts)} cases -> default +sweep.schedule = {"population" if all(verdicts) else "per_learner"}')


if __name__ == '__main__':
  main()
