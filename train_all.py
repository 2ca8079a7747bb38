"""`python train_all.py algorithm=<ALG> [key=value ...]`: one algorithm on ant, halfcheetah, hopper and walker2d at once (reference train_all.py:16-28 and
conf/train_all_config.yaml); prints the four mean normalised scores and returns their minimum - the objective the reference hands its hyperparameter search.

The configuration is composed ONCE (il.config.compose, as `train.py` composes it) and copied per environment with `env` overwritten. All four share one seed: the `seed=`
override if one is given, otherwise `random.randint(0, 99)` as in the reference, printed. (The reference ALWAYS draws, whatever `seed=` says; honouring the override is a
deliberate difference - it is what makes a run repeatable.) Outputs go to outputs/<ALG>_all/<time>/<env>/... (the reference's `file_prefix=f'{env}/'`).

The reference trains the four in four processes. Here they train in ONE process, in lockstep, as a population of four learners of different state / action widths
(`train.train_sweep(..., vary_env=True)`):
  +sweep.schedule=population   (default: profiles/train_all_ab.txt) one acting launch per lockstep environment step and one set of update launches per update for all four (il.PopulationActingWorker and
                               il.BatchedPopulationPlan over learners of different widths: the `_mixed` entry points of include/il_hip.h);
  +sweep.schedule=per_learner  the same driver, learners and seeds through one ActingWorker and one plan.run() per learner: the A/B partner, and the same bits.
Configurations the population launches do not serve at different widths (PWIL, AdRIL, RED, GMMIL, DRIL, BC, GAIL with Mixup, general shapes, ...:
`train.mixed_env_fallback_reason`) train environment after environment through `train()` under the same prefixes; a `[train_all]` line on stderr gives the reason.
`+evaluation.schedule=lockstep` (default `sequential`) is train.py's key and is passed through: every learner then evaluates on `evaluation.episodes` seeded copies of its
evaluation environment, one il_act_eval_rows launch per lockstep step for all learners and episodes (per learner under `per_learner` and in the fallback).

`python train_all.py -m key=a,b,... algorithm=<ALG>`: the jobs are expanded like Hydra's BASIC sweeper (il.config.compose_multirun: the Cartesian product of the comma
lists). The reference's train_all_config.yaml selects the Ax sweeper and reads conf/hyperparameter_search_space/<ALG>.yaml; neither exists here: no Ax, and
`hyperparameter_search_space` is not read. Job j writes to outputs/<ALG>_all_sweeper/<time>/<j>/<env>/. Jobs that differ only in `seed` form ONE population of 4 x K
learners; other jobs run one after another, each as its own four-environment population. Every job's minimum score is printed, the best job last."""
import copy
import os
import random
import sys
import time

import numpy as np

import train as T
from imitation_learning_amd import config as il_config

ENVS = list(il_config.ENVS)   # ant, halfcheetah, hopper, walker2d (reference environments.py ENVS)
DEFAULT_SCHEDULE = 'population'   # measured (profiles/train_all_ab.txt): 1.7 - 3.3x per_learner's aggregate env-steps/s at 4 and at 16 learners, SAC and GAIL, far beyond its spread

HELP = __doc__


def env_configs(cfg, seed: int):
  """One copy of the composed configuration per environment, `env` and `seed` overwritten (reference train_all.py:20-24)."""
  out = []
  for env in ENVS:
    c = copy.deepcopy(cfg)
    c.env, c.seed = env, int(seed)
    if (c.get('sweep', {}) or {}).get('schedule') is None:   # train_all.py's own default; an explicit +sweep.schedule wins
      c['sweep'] = dict(c.get('sweep', {}) or {}, schedule=DEFAULT_SCHEDULE)
    out.append(c)
  return out


def _has_seed(overrides) -> bool:
  return any(o.partition('=')[0].lstrip('+') == 'seed' for o in overrides)


def pick_seed(overrides, cfg, rng=random) -> int:
  """The `seed=` override if given, else the reference's draw (train_all.py:19), printed so that the run can be repeated."""
  if _has_seed(overrides): return int(cfg.seed)
  seed = rng.randint(0, 99)
  print(f'[train_all] no seed= given: drew seed={seed} for all environments (pass seed={seed} to repeat this run)')
  return seed


def run_dir(cfg, stamp: str) -> str:
  """The reference's hydra.run.dir of train_all_config.yaml: outputs/${algorithm}_all/<time>."""
  return os.path.join('outputs', f'{cfg.algorithm}_all', stamp)


def sweep_dir(cfg, stamp: str) -> str:
  """hydra.sweep.dir of train_all_config.yaml: outputs/${algorithm}_all_sweeper/<time>; job n writes into its subdirectory n."""
  return os.path.join('outputs', f'{cfg.algorithm}_all_sweeper', stamp)


def fallback_reason(cfgs):
  """None when these per-environment configurations can train as one population; otherwise the reason they train one after another through train()."""
  for c in cfgs:
    reason = T.mixed_env_fallback_reason(c)
    if reason is not None: return reason
  return None


def job_groups(cfgs):
  """The jobs of `train_all.py -m` as runs: [(job numbers, reason)] in job order. reason None with several jobs: they differ only in `seed` and train as one population of
  4 x len(jobs) learners; reason None with one job: its own four-environment population; otherwise one job whose environments train one after another."""
  keys, members = [], []
  for j, cfg in enumerate(cfgs):
    k = T._without_seed(cfg, ('env',))
    for i, other in enumerate(keys):
      if other == k:
        members[i].append(j); break
    else:
      keys.append(k); members.append([j])
  runs = []
  for jobs in members:
    reason = fallback_reason(env_configs(cfgs[jobs[0]], cfgs[jobs[0]].seed))
    together = reason is None and len({int(cfgs[j].seed) for j in jobs}) == len(jobs)   # two jobs with one seed would be one learner twice: each on its own then
    runs += [(jobs, reason)] if together else [([j], reason) for j in jobs]
  return sorted(runs, key=lambda r: r[0][0])


def _train_envs(cfgs, prefixes, what: str):
  """The learners of `cfgs` (one per environment and job) as one population, or - with a fallback reason - one after another through train(). Scores in order."""
  reason = fallback_reason(cfgs)
  if reason is None:
    print(f'[train_all] {what}: {len(cfgs)} learners ({", ".join(f"{c.env} seed={c.seed}" for c in cfgs)}) train as one population (+sweep.schedule={T.sweep_schedule(cfgs[0])})', file=sys.stderr)
    return T.train_sweep(cfgs, prefixes, vary_env=True, noise_ids=[ENVS.index(c.env) for c in cfgs])   # a job's learners draw the same noise alone and beside other jobs
  print(f'[train_all] {what}: the environments train one after another: {reason}', file=sys.stderr)
  return [T.train(c, file_prefix=p) for c, p in zip(cfgs, prefixes)]


def train_all(argv, stamp=None):
  """`python train_all.py ...` without -m. Returns (run directory, {env: mean normalised score}, their minimum)."""
  cfg = il_config.compose(list(argv))
  seed = pick_seed(argv, cfg)
  cfgs = env_configs(cfg, seed)
  root = os.path.abspath(run_dir(cfg, stamp or time.strftime('%m-%d_%H-%M-%S')))
  prefixes = []
  for env in ENVS:
    os.makedirs(os.path.join(root, env), exist_ok=True)   # a new folder per environment (train_all.py:25)
    prefixes.append(os.path.join(root, env, ''))
  scores = dict(zip(ENVS, _train_envs(cfgs, prefixes, f'algorithm={cfg.algorithm} seed={seed}')))
  for env in ENVS:
    print(f'{cfg.algorithm} {env}: mean normalised score {scores[env]:.4f} (outputs in {os.path.join(root, env)})')
  worst = min(scores.values())
  print(f'{cfg.algorithm} all: minimum mean normalised score {worst:.4f}')
  return root, scores, worst


def multirun(argv, stamp=None):
  """`python train_all.py -m ...`. Returns (sweep directory, [{env: score} per job], [minimum per job])."""
  cfgs, overrides = il_config.compose_multirun(list(argv))
  if not _has_seed(overrides[0]):
    seed = pick_seed(overrides[0], cfgs[0])
    for c in cfgs: c.seed = seed
  root = os.path.abspath(sweep_dir(cfgs[0], stamp or time.strftime('%m-%d_%H-%M-%S')))
  prefixes = [[os.path.join(root, str(j), env, '') for env in ENVS] for j in range(len(cfgs))]
  for job in prefixes:
    for p in job: os.makedirs(p, exist_ok=True)
  scores = [None] * len(cfgs)
  for jobs, reason in job_groups(cfgs):
    members = [(j, c, p) for j in jobs for c, p in zip(env_configs(cfgs[j], cfgs[j].seed), prefixes[j])]
    out = _train_envs([c for _, c, _ in members], [p for _, _, p in members], f'jobs {jobs[0]}..{jobs[-1]}' if len(jobs) > 1 else f'job {jobs[0]}')
    for (j, c, _), sc in zip(members, out):
      scores[j] = dict(scores[j] or {}, **{c.env: sc})
  worst = [min(s.values()) for s in scores]
  for j, s in enumerate(scores):
    print(f'#{j} {" ".join(overrides[j])}: ' + ', '.join(f'{env} {s[env]:.4f}' for env in ENVS) + f': minimum {worst[j]:.4f} (outputs in {os.path.join(root, str(j))})')
  finite = [j for j in range(len(cfgs)) if np.isfinite(worst[j])]
  if finite:
    best = max(finite, key=lambda j: worst[j])
    print(f'best: #{best} {" ".join(overrides[best])}: minimum mean normalised score {worst[best]:.4f}')
  return root, scores, worst


def main(argv):
  if any(o in ('-h', '--help') for o in argv):
    print(HELP)
    return None
  if any(o in ('-m', '--multirun') for o in argv):
    return multirun(argv)[2]
  return train_all(argv)[2]


if __name__ == '__main__':
  main(sys.argv[1:])
