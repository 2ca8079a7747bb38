"""`python train.py -m ...` without a GPU: the multirun expansion (Hydra's basic sweeper: comma lists, Cartesian product, last key fastest), which jobs of a sweep form a
population and which run one after another (and why), and the sweep directory layout."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imitation_learning_amd import config  # noqa: E402


def test_multirun_expands_comma_lists_in_hydra_order():
  cfgs, jobs = config.compose_multirun(['-m', 'seed=1,2,3', 'algorithm=GAIL', 'env=hopper,ant'])
  assert jobs == [[f'seed={s}', 'algorithm=GAIL', f'env={e}'] for s in (1, 2, 3) for e in ('hopper', 'ant')]   # the last swept key varies fastest
  assert [(c.seed, c.env) for c in cfgs] == [(s, e) for s in (1, 2, 3) for e in ('hopper', 'ant')]
  assert all(c.algorithm == 'GAIL' and c.reinforcement.discount == 0.97 for c in cfgs)
  cfgs, jobs = config.compose_multirun(['--multirun', 'seed=7', 'training.batch_size=64, 128'])
  assert [c.training.batch_size for c in cfgs] == [64, 128] and jobs[1] == ['seed=7', 'training.batch_size=128']
  cfgs, jobs = config.compose_multirun(['-m', 'algorithm=SAC'])
  assert len(cfgs) == 1 and jobs == [['algorithm=SAC']]


def test_multirun_sweeps_added_keys_and_keeps_bracketed_values_whole():
  cfgs, jobs = config.compose_multirun(['-m', '+sweep.schedule=population,per_learner', '+acting.schedule=fused', 'seed=1,2', '+extra.list=[1,2]'])
  assert [(c.sweep.schedule, c.seed) for c in cfgs] == [(s, k) for s in ('population', 'per_learner') for k in (1, 2)]
  assert all(c.acting.schedule == 'fused' and c.extra.list == [1, 2] for c in cfgs)
  assert jobs[0] == ['+sweep.schedule=population', '+acting.schedule=fused', 'seed=1', '+extra.list=[1,2]']


@pytest.mark.parametrize('flag', ['-m', '--multirun'])
def test_compose_still_refuses_multirun(flag):
  with pytest.raises(NotImplementedError):
    config.compose([flag, 'seed=1,2'])


def _groups(argv):
  import train
  cfgs, _ = config.compose_multirun(['-m'] + argv)
  for c in cfgs: config.validate(c)
  return train.sweep_groups(cfgs)


def test_seed_only_jobs_form_one_population():
  for argv in (['seed=1,2,3', 'algorithm=GAIL', 'env=halfcheetah'], ['seed=4,9', 'algorithm=SAC', '+acting.schedule=fused'], ['seed=1,2', 'algorithm=GAIL', 'bc_pretraining.iterations=10'],
               ['seed=1,2', 'algorithm=GAIL', 'imitation.loss_function=PUGAIL'], ['seed=1,2', 'algorithm=SAC', 'reinforcement.actor.hidden_size=128', 'reinforcement.critic.hidden_size=128']):
    runs = _groups(argv)
    assert len(runs) == 1 and runs[0][1] is None and runs[0][0] == list(range(len(runs[0][0]))), argv
  # two environments x two seeds: one population per environment, in job order
  runs = _groups(['env=hopper,ant', 'seed=1,2', 'algorithm=SAC'])
  assert runs == [([0, 1], None), ([2, 3], None)]
  runs = _groups(['seed=1,2', 'env=hopper,ant', 'algorithm=SAC'])
  assert runs == [([0, 2], None), ([1, 3], None)]


@pytest.mark.parametrize('argv,word', [
    (['algorithm=PWIL'], 'algorithm=PWIL'), (['algorithm=AdRIL'], 'algorithm=AdRIL'), (['algorithm=GMMIL'], 'GMMIL'), (['algorithm=BC'], 'BC'),
    (['algorithm=GAIL', 'imitation.discriminator.subtract_log_policy=true'], 'subtract_log_policy'), (['algorithm=GAIL', 'imitation.discriminator.reward_shaping=true'], 'reward shaping'),
    (['algorithm=GAIL', 'imitation.discriminator.depth=2'], 'discriminator'), (['algorithm=GAIL', 'imitation.discriminator.activation=tanh'], 'discriminator'),
    (['algorithm=GAIL', 'imitation.loss_function=PUGAIL', 'imitation.nonnegative_margin=0.05'], 'margin'),
    (['algorithm=GAIL', 'imitation.loss_function=Mixup', 'imitation.mixup_alpha=0.5'], 'Mixup'), (['algorithm=GAIL', 'imitation.loss_function=Mixup'], 'Mixup'),
    (['algorithm=GAIL', 'imitation.loss_function=Mixup', 'imitation.mixup_alpha=1'], 'Mixup'),
    (['algorithm=SAC', 'reinforcement.actor.depth=3'], 'shape'), (['algorithm=SAC', 'reinforcement.critic.activation=tanh'], 'shape'), (['algorithm=SAC', 'reinforcement.actor.hidden_size=320', 'reinforcement.critic.hidden_size=320'], 'shape'),
    (['algorithm=SAC', 'training.batch_size=100'], 'multiple of 16'), (['algorithm=GAIL', 'imitation.mix_expert_data=mixed_batch'], 'mix_expert_data'),
    (['algorithm=GAIL', 'imitation.bc_aux_loss=true'], 'bc_aux_loss'), (['algorithm=SAC', 'distributed.world_size=2'], 'world_size'),
    (['algorithm=SAC', '+acting.schedule=overlap'], 'acting.schedule'), (['algorithm=SAC', '+acting.schedule=per_function'], 'acting.schedule')])
def test_configurations_without_population_launches_run_job_after_job(argv, word):
  runs = _groups(['seed=1,2'] + argv)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  assert all(reason is not None and word in reason for _, reason in runs), runs


def test_single_jobs_and_repeated_seeds_do_not_form_a_population():
  runs = _groups(['seed=1', 'algorithm=SAC', 'training.batch_size=64,128'])
  assert [jobs for jobs, _ in runs] == [[0], [1]] and all('seed alone' in reason for _, reason in runs)
  runs = _groups(['seed=1,1', 'algorithm=SAC'])
  assert [jobs for jobs, _ in runs] == [[0], [1]] and all('same seed' in reason for _, reason in runs)


def test_sweep_schedule_key():
  import train
  assert train.sweep_schedule(config.compose(['+sweep.schedule=population'])) == 'population'
  assert train.sweep_schedule(config.compose(['+sweep.schedule=per_learner'])) == 'per_learner'
  assert train.sweep_schedule(config.compose([])) == train.SWEEP_DEFAULT_SCHEDULE and train.SWEEP_DEFAULT_SCHEDULE in train.SWEEP_SCHEDULES
  with pytest.raises(AssertionError):
    train.sweep_schedule(config.compose(['+sweep.schedule=round_robin']))


def test_sweep_directory_layout(tmp_path, monkeypatch, capsys):
  """outputs/<algorithm>_<env>_sweeper/<time>/<job number>/ (the reference's hydra.sweep.dir); populations go to train_sweep with one prefix per job, the rest to train(),
  each with its `[train] sweep:` line."""
  import train
  calls = []
  monkeypatch.setattr(train, 'train_sweep', lambda cfgs, prefixes: (calls.append(('sweep', [c.seed for c in cfgs], prefixes)), [0.5] * len(cfgs))[1])
  monkeypatch.setattr(train, 'train', lambda cfg, file_prefix='': (calls.append(('train', cfg.seed, file_prefix)), 0.25)[1])
  monkeypatch.chdir(tmp_path)
  assert train.sweep_dir(config.compose(['algorithm=GAIL', 'env=hopper']), 'T') == os.path.join('outputs', 'GAIL_hopper_sweeper', 'T')
  scores = train.main(['-m', 'seed=1,2,3', 'algorithm=GAIL', 'env=hopper'])
  assert scores == [0.5, 0.5, 0.5]
  sweeper = tmp_path / 'outputs' / 'GAIL_hopper_sweeper'
  stamp, = os.listdir(sweeper)
  import re
  assert re.fullmatch(r'\d\d-\d\d_\d\d-\d\d-\d\d', stamp), stamp   # %m-%d_%H-%M-%S, as the reference's hydra.sweep.dir and the single run's directory
  assert sorted(os.listdir(sweeper / stamp)) == ['0', '1', '2']
  assert calls == [('sweep', [1, 2, 3], [os.path.join(str(sweeper / stamp), str(j), '') for j in range(3)])]
  err = capsys.readouterr().err
  assert err.count('[train] sweep:') == 1 and 'one population of 3 learners' in err
  calls.clear()
  root, scores = train.multirun(['-m', 'seed=1,2', 'algorithm=PWIL', 'env=walker2d'], stamp='T')
  assert root == str(tmp_path / 'outputs' / 'PWIL_walker2d_sweeper' / 'T') and scores == [0.25, 0.25]
  assert calls == [('train', 1, os.path.join(root, '0', '')), ('train', 2, os.path.join(root, '1', ''))]
  err = capsys.readouterr().err
  assert err.count('[train] sweep:') == 2 and 'one job after another' in err and 'PWIL' in err


def test_train_sweep_refuses_what_is_not_a_population():
  import train
  cfgs, _ = config.compose_multirun(['-m', 'seed=1,2', 'algorithm=PWIL', 'steps=10'])
  with pytest.raises(NotImplementedError, match='PWIL'):
    train.train_sweep(cfgs, ['a/', 'b/'])
  cfgs, _ = config.compose_multirun(['-m', 'seed=1,2', 'env=hopper,ant', 'steps=10'])
  with pytest.raises(AssertionError, match='only in their seed'):
    train.train_sweep(cfgs[:2], ['a/', 'b/'])
