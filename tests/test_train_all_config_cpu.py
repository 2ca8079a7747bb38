"""`python train_all.py ...` without a GPU: the per-environment configurations (composed once, copied with `env` and one seed overwritten), the seed rule (the override,
or a printed draw from 0..99), the directory layout (outputs/<ALG>_all/<time>/<env>/ and outputs/<ALG>_all_sweeper/<time>/<job>/<env>/), which jobs of `-m` form one
population, the configurations that train environment after environment (and why), the descriptor of the mixed acting launch against a C program compiled with
include/il_hip.h - and that `train.py -m env=a,b` keeps grouping per environment."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from imitation_learning_amd import config  # noqa: E402


def test_env_configs_are_one_composition_copied_per_environment():
  import train_all
  cfg = config.compose(['algorithm=GAIL', 'seed=3', 'training.batch_size=64', 'env=hopper'])
  cfgs = train_all.env_configs(cfg, 3)
  assert train_all.ENVS == ['ant', 'halfcheetah', 'hopper', 'walker2d'] == [c.env for c in cfgs]
  assert all(c.seed == 3 and c.algorithm == 'GAIL' and c.training.batch_size == 64 and c.reinforcement.discount == 0.97 for c in cfgs)
  assert cfg.env == 'hopper', 'the composed configuration itself is left alone'
  import train
  assert train_all.DEFAULT_SCHEDULE in train.SWEEP_SCHEDULES and all(train.sweep_schedule(c) == train_all.DEFAULT_SCHEDULE for c in cfgs), 'train_all.py has a default schedule of its own'
  explicit = train_all.env_configs(config.compose(['algorithm=GAIL', '+sweep.schedule=per_learner']), 3)
  assert all(train.sweep_schedule(c) == 'per_learner' for c in explicit), 'an explicit +sweep.schedule wins'
  assert train.sweep_schedule(config.compose(['algorithm=GAIL'])) == train.SWEEP_DEFAULT_SCHEDULE == 'per_learner', 'the seed sweeps of train.py keep their default'
  cfgs[0].training.batch_size = 128
  assert cfgs[1].training.batch_size == 64 and cfg.training.batch_size == 64, 'copies, not views'
  import train
  assert all(train._without_seed(c, ('env',)) == train._without_seed(cfgs[1], ('env',)) for c in cfgs[1:])


def test_seed_is_the_override_or_a_printed_draw(capsys):
  import train_all

  class Rng:
    def randint(self, lo, hi):
      assert (lo, hi) == (0, 99)
      return 41
  assert train_all.pick_seed(['algorithm=SAC', 'seed=7'], config.compose(['algorithm=SAC', 'seed=7']), Rng()) == 7
  assert capsys.readouterr().out == ''
  assert train_all.pick_seed(['algorithm=SAC'], config.compose(['algorithm=SAC']), Rng()) == 41
  assert 'seed=41' in capsys.readouterr().out
  assert train_all.pick_seed(['algorithm=SAC', 'seed=0'], config.compose(['algorithm=SAC', 'seed=0']), Rng()) == 0, 'seed=0 is an override, not a missing one'


@pytest.mark.parametrize('argv,word', [
    (['algorithm=PWIL'], 'PWIL'), (['algorithm=AdRIL'], 'AdRIL'), (['algorithm=GMMIL'], 'GMMIL'), (['algorithm=BC'], 'BC'), (['algorithm=DRIL'], 'DRIL'),
    (['algorithm=RED'], 'different state / action widths'), (['algorithm=GMMIL', '+sweep.schedule=population'], 'different state / action widths'),
    (['algorithm=DRIL', '+sweep.schedule=population'], 'different state / action widths'), (['algorithm=PWIL', '+sweep.pwil_population=true'], 'different state / action widths'),
    (['algorithm=GAIL', 'imitation.loss_function=Mixup'], 'Mixup'), (['algorithm=GAIL', 'imitation.loss_function=Mixup', '+sweep.gail_mixup_population=true'], 'Mixup'),
    (['algorithm=SAC', 'reinforcement.actor.depth=3'], 'shape'), (['algorithm=SAC', 'reinforcement.actor.hidden_size=128'], 'different hidden sizes'),
    (['algorithm=SAC', 'training.batch_size=100'], 'multiple of 16'), (['algorithm=GAIL', 'imitation.bc_aux_loss=true'], 'bc_aux_loss'),
    (['algorithm=GAIL', 'imitation.discriminator.reward_shaping=true'], 'reward shaping'), (['algorithm=SAC', '+acting.schedule=overlap'], 'acting.schedule')])
def test_configurations_that_train_environment_after_environment(argv, word):
  import train_all
  cfg = config.compose(argv + ['seed=1'])
  reason = train_all.fallback_reason(train_all.env_configs(cfg, 1))
  assert reason is not None and word in reason, reason


@pytest.mark.parametrize('argv', [['algorithm=SAC'], ['algorithm=GAIL'], ['algorithm=GAIL', 'imitation.loss_function=PUGAIL'], ['algorithm=SAC', '+acting.schedule=fused'],
                                  ['algorithm=SAC', 'reinforcement.actor.hidden_size=64', 'reinforcement.critic.hidden_size=64', 'training.batch_size=64']])
def test_configurations_that_train_as_one_mixed_population(argv):
  import train_all
  assert train_all.fallback_reason(train_all.env_configs(config.compose(argv), 1)) is None


def _fake_training(monkeypatch):
  import train
  calls = []

  def sweep(cfgs, prefixes, vary_env=False, noise_ids=None):
    calls.append(('sweep', [(c.env, c.seed) for c in cfgs], list(prefixes), vary_env, noise_ids))
    return [0.1 * (1 + train.il_config.ENVS.index(c.env)) + 0.01 * c.seed for c in cfgs]
  monkeypatch.setattr(train, 'train_sweep', sweep)
  monkeypatch.setattr(train, 'train', lambda cfg, file_prefix='': (calls.append(('train', cfg.env, cfg.seed, file_prefix)), 0.5 if cfg.env != 'hopper' else 0.25)[1])
  return calls


def test_run_directory_layout_result_and_fallback(tmp_path, monkeypatch, capsys):
  import train_all
  calls = _fake_training(monkeypatch)
  monkeypatch.chdir(tmp_path)
  worst = train_all.main(['algorithm=SAC', 'seed=3', '+sweep.schedule=population'])
  base = tmp_path / 'outputs' / 'SAC_all'
  stamp, = os.listdir(base)
  assert re.fullmatch(r'\d\d-\d\d_\d\d-\d\d-\d\d', stamp), stamp
  assert sorted(os.listdir(base / stamp)) == ['ant', 'halfcheetah', 'hopper', 'walker2d']
  envs = ['ant', 'halfcheetah', 'hopper', 'walker2d']
  assert calls == [('sweep', [(e, 3) for e in envs], [os.path.join(str(base / stamp), e, '') for e in envs], True, [0, 1, 2, 3])]
  assert worst == pytest.approx(0.13)   # the minimum of the four
  out, err = capsys.readouterr()
  assert all(f'SAC {e}: mean normalised score' in out for e in envs) and out.rstrip().endswith('SAC all: minimum mean normalised score 0.1300')
  assert err.count('[train_all]') == 1 and 'train as one population' in err and '+sweep.schedule=population' in err
  # a configuration without mixed-width population launches: environment after environment through train(), the reason on stderr, the same prefixes
  calls.clear()
  root, scores, worst = train_all.train_all(['algorithm=PWIL', 'seed=5'], stamp='T')
  assert root == str(tmp_path / 'outputs' / 'PWIL_all' / 'T')
  assert calls == [('train', e, 5, os.path.join(root, e, '')) for e in envs]
  assert scores == dict(ant=0.5, halfcheetah=0.5, hopper=0.25, walker2d=0.5) and worst == 0.25
  err = capsys.readouterr().err
  assert err.count('[train_all]') == 1 and 'one after another' in err and 'algorithm=PWIL has no population launches' in err
  # without seed=: one draw from 0..99 for all four, printed
  calls.clear()
  train_all.train_all(['algorithm=SAC'], stamp='U')
  (_, learners, _, _, _), = calls
  assert len({s for _, s in learners}) == 1 and 0 <= learners[0][1] <= 99
  assert f'drew seed={learners[0][1]}' in capsys.readouterr().out


def test_multirun_groups_jobs_and_lays_out_the_sweep_directory(tmp_path, monkeypatch, capsys):
  import train_all
  calls = _fake_training(monkeypatch)
  monkeypatch.chdir(tmp_path)
  envs = ['ant', 'halfcheetah', 'hopper', 'walker2d']
  root, scores, worst = train_all.multirun(['-m', 'seed=3,4', 'algorithm=SAC', '+sweep.schedule=population'], stamp='T')
  assert root == str(tmp_path / 'outputs' / 'SAC_all_sweeper' / 'T') and sorted(os.listdir(root)) == ['0', '1']
  assert all(sorted(os.listdir(os.path.join(root, j))) == envs for j in ('0', '1'))
  # the two jobs differ only in their seed: ONE population of eight learners, job-major, each learner's noise id its environment's
  assert calls == [('sweep', [(e, s) for s in (3, 4) for e in envs], [os.path.join(root, str(j), e, '') for j in (0, 1) for e in envs], True, [0, 1, 2, 3] * 2)]
  assert worst == [pytest.approx(0.13), pytest.approx(0.14)] and [sorted(s) for s in scores] == [envs, envs]
  out = capsys.readouterr().out
  assert out.index('#0 seed=3') < out.index('#1 seed=4') < out.index('best: #1 seed=4')
  # jobs that differ in something else: one four-environment population each, one after another
  calls.clear()
  train_all.multirun(['-m', 'seed=3', 'algorithm=SAC', 'training.batch_size=64,128'], stamp='V')
  assert [(c[0], len(c[1]), c[4]) for c in calls] == [('sweep', 4, [0, 1, 2, 3])] * 2
  import train
  cfgs, _ = config.compose_multirun(['-m', 'seed=1,2', 'training.batch_size=64,128', 'algorithm=GAIL'])
  assert [jobs for jobs, _ in train_all.job_groups(cfgs)] == [[0, 2], [1, 3]]
  cfgs, _ = config.compose_multirun(['-m', 'seed=1,1', 'algorithm=SAC'])
  assert [jobs for jobs, _ in train_all.job_groups(cfgs)] == [[0], [1]]
  cfgs, _ = config.compose_multirun(['-m', 'seed=1,2', 'algorithm=PWIL'])
  runs = train_all.job_groups(cfgs)
  assert [jobs for jobs, _ in runs] == [[0], [1]] and all('PWIL' in reason for _, reason in runs)


def test_help_names_what_is_not_read(capsys):
  import train_all
  assert train_all.main(['--help']) is None
  out = capsys.readouterr().out
  assert 'hyperparameter_search_space' in out and 'Ax' in out and 'seed' in out


def test_train_sweep_keeps_its_seed_only_rule_and_train_py_keeps_grouping_per_env(tmp_path, monkeypatch, capsys):
  """`train.py -m env=hopper,ant seed=1,2` forms one population per environment, as before; train_sweep refuses jobs of different environments unless its caller says
  they may differ (train_all.py), and then refuses what has no launches for different widths."""
  import train
  cfgs, _ = config.compose_multirun(['-m', 'env=hopper,ant', 'seed=1,2', 'algorithm=SAC'])
  for c in cfgs: config.validate(c)
  assert train.sweep_groups(cfgs) == [([0, 1], None), ([2, 3], None)]
  # ... and through the entry point itself: train.multirun hands train_sweep one population per environment, with its two positional arguments as before
  calls = []
  monkeypatch.setattr(train, 'train_sweep', lambda cfgs, prefixes: (calls.append(('sweep', [(c.env, c.seed) for c in cfgs], prefixes)), [0.5] * len(cfgs))[1])
  monkeypatch.setattr(train, 'train', lambda cfg, file_prefix='': (calls.append(('train', cfg.env, cfg.seed, file_prefix)), 0.25)[1])
  monkeypatch.chdir(tmp_path)
  root, scores = train.multirun(['-m', 'env=hopper,ant', 'seed=1,2', 'algorithm=SAC', 'steps=10'], stamp='T')
  job = lambda j: os.path.join(root, str(j), '')
  assert calls == [('sweep', [('hopper', 1), ('hopper', 2)], [job(0), job(1)]), ('sweep', [('ant', 1), ('ant', 2)], [job(2), job(3)])] and scores == [0.5] * 4
  err = capsys.readouterr().err
  assert err.count('[train] sweep:') == 2 and err.count('one population of 2 learners') == 2
  monkeypatch.undo()
  cfgs, _ = config.compose_multirun(['-m', 'seed=1,2', 'env=hopper,ant', 'steps=10'])
  with pytest.raises(AssertionError, match='only in their seed'):
    train.train_sweep(cfgs[:2], ['a/', 'b/'])
  cfgs, _ = config.compose_multirun(['-m', 'seed=1', 'env=hopper,ant', 'training.batch_size=64,128', 'steps=10'])
  with pytest.raises(AssertionError, match='only in seed and env'):
    train.train_sweep([cfgs[0], cfgs[3]], ['a/', 'b/'], vary_env=True)
  cfgs, _ = config.compose_multirun(['-m', 'seed=1', 'env=hopper,ant', 'algorithm=RED', 'steps=10'])
  with pytest.raises(NotImplementedError, match='different state / action widths'):
    train.train_sweep(cfgs, ['a/', 'b/'], vary_env=True)


def test_act_dims_descriptor_matches_the_header(tmp_path):
  """il_act_dims - the per-learner record of il_act_step_population_mixed - against a C program compiled with include/il_hip.h: size and every offset. il_act_learner and
  il_struct_size are what they were (the new record has no il_struct_size number)."""
  from imitation_learning_amd import _lib
  from test_sweep_gmmil_config_cpu import _c_compiler
  cc = _c_compiler()
  lang = ['-x', 'c'] if os.path.basename(cc) == 'hipcc' else []
  src = tmp_path / 'layout.c'
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "il_hip.h"\nint main(void) {\n'
                 '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(il_act_dims), offsetof(il_act_dims, state_dim), offsetof(il_act_dims, action_dim), offsetof(il_act_dims, ring_row_floats),\n'
                 '         offsetof(il_act_dims, reserved), sizeof(il_act_learner));\n  return 0;\n}\n')
  exe = tmp_path / 'layout'
  subprocess.run([cc] + lang + ['-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
  got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
  D = _lib.ActDims
  assert got == [C.sizeof(D), D.state_dim.offset, D.action_dim.offset, D.ring_row_floats.offset, D.reserved.offset, C.sizeof(_lib.ActLearner)] == [16, 0, 4, 8, 12, 48]
  names = set(_lib._SIGNATURES)
  assert {'il_sac_update_population_mixed', 'il_act_step_population_mixed', 'il_gail_step_population_mixed'} <= names
