"""The population acting launch (il_act_step_population: k_act_step_population) and il.PopulationActingWorker on the host emulation of the kernels (tests/host_emu): the
bodies of tests/test_population_acting_gpu.py with the library handle swapped for the emulation, as tests/test_acting_general_emulated.py runs its GPU bodies. The
emulator's lanes do not run in lockstep, and under IL_EMU_SCHEDULE its waves and the workgroups of a launch run in a shuffled order:
test_population_acting_does_not_depend_on_the_schedule re-runs the kernel-level cases of this file that way, so the 235-float rows of the (111, 8, 64, 9) case are the
regression test for the commit order: cursor and consumed word behind the last barrier, echo last, per learner."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402


class _Event:   # torch.cuda.Event (il.PretrainPlan records one per copy): the emulated null stream runs every copy at once
  def record(self, *a, **k): pass
  def synchronize(self): pass


def _bodies(monkeypatch):
  """tests/test_population_acting_gpu.py with its GPU-only names bound to the CPU and the emulated library."""
  import torch
  import gpu_util
  tgp = E._emulated_product(monkeypatch, streams=True)
  monkeypatch.setattr(torch.cuda, 'Event', _Event)
  import test_population_acting_gpu as tp
  for k in ('DEV', 'N', 'Cfg'):
    monkeypatch.setattr(tp, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tgp.il), ('_lib', _lib)):
    monkeypatch.setattr(tp, k, v, raising=False)
  return tp


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
@pytest.mark.parametrize('shape', [(18, 6, 64, 3), (111, 8, 64, 9)], ids=['S18-A6-H64-L3', 'S111-A8-H64-L9'])
def test_population_acting_matches_per_learner_workers_on_the_emulated_kernels(monkeypatch, shape, schedule, absorbing):
  _bodies(monkeypatch).test_population_acting_matches_per_learner_workers(shape, schedule, absorbing)


@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_population_acting_idle_learner_and_repeated_launches_on_the_emulated_kernels(monkeypatch, schedule):
  _bodies(monkeypatch).test_population_acting_idle_learner_and_repeated_launches(schedule)


def test_population_greedy_and_evaluate_population_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_population_greedy_and_evaluate_population()


def test_population_acting_loud_failures_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_population_acting_loud_failures()


def test_act_learner_descriptor_abi_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_act_learner_descriptor_abi()


SHORT = ['steps=140', 'training.start=120', 'evaluation.interval=70', 'evaluation.episodes=1', 'logging.interval=10', '+synthetic_env.max_episode_steps=60', '+synthetic_env.dataset_trajectories=6',
         'training.batch_size=64',   # (tests/test_acting_general_emulated.py SHORT)
         'reinforcement.actor.hidden_size=64', 'reinforcement.critic.hidden_size=64']   # the smallest fused shape: the emulated MFMAs are what these runs spend their time in


KERNEL_LEVEL = 'population_acting_matches or idle_learner or evaluate_population'   # the 11 cases above that launch the kernel


def test_population_acting_does_not_depend_on_the_schedule():
  """The kernel-level cases above with the waves of every workgroup, the lanes of every wave and the workgroups of every launch in a random order (IL_EMU_SCHEDULE is read
  once per process, hence the child): a learner's append, cursor and echo must not depend on which wave or which learner's workgroup runs first."""
  import subprocess
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k', KERNEL_LEVEL], env=dict(os.environ, IL_EMU_SCHEDULE='random:3'),
                     cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=1500)
  assert r.returncode == 0 and '11 passed' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize('extra', [[], ['imitation.loss_function=PUGAIL', 'bc_pretraining.iterations=4']], ids=['BCE', 'PUGAIL-bc-pretraining'])
def test_seed_sweep_population_equals_per_learner_on_the_emulated_kernels(monkeypatch, tmp_path, extra):
  """tests/test_population_acting_gpu.py::test_seed_sweep_population_equals_per_learner, shortened: `-m seed=3,4 algorithm=GAIL env=hopper` under both sweep schedules; then
  with a GAIL loss other than BCE (PUGAIL, infinite margin) and a BC pretraining plan per learner in front of the loop."""
  import numpy as np
  import torch
  tp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  argv = ['-m', 'seed=3,4', 'algorithm=GAIL', 'env=hopper'] + SHORT + extra
  root_p, scores_p = tp._sweep(tmp_path, 'population', argv + ['+sweep.schedule=population'])
  root_l, scores_l = tp._sweep(tmp_path, 'per_learner', argv + ['+sweep.schedule=per_learner'])
  assert np.isfinite(scores_p).all() and scores_p == scores_l
  for j in (0, 1):
    fp, fl = tp._job_files(root_p, j), tp._job_files(root_l, j)
    assert set(fp) == set(fl) == {'agent.pth', 'discriminator.pth', 'metrics.pth'}
    for f in fp:
      a, b = ({k: v for k, v in m.items() if k not in tp.TIMING_KEYS} for m in (fp[f], fl[f]))
      tp._assert_same_nested(a, b, f'job {j}: {f}')
    assert len(fp['metrics.pth']['update_steps']) >= 1 and len(fp['metrics.pth']['test_steps']) == 2
  a0, a1 = (tp._job_files(root_p, j)['agent.pth']['actor'] for j in (0, 1))
  assert any(not torch.equal(v, a1[k]) for k, v in a0.items())


def test_seed_sweep_graph_replays_equal_direct_launches_on_the_emulated_kernels(monkeypatch, tmp_path):
  tp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  tp.test_seed_sweep_graph_replays_equal_direct_launches(tmp_path, monkeypatch, short=SHORT)


def test_seed_sweep_at_a_ragged_batch_trains_job_after_job_on_the_emulated_kernels(monkeypatch, tmp_path, capsys):
  """`python train.py -m seed=3,4 algorithm=SAC training.batch_size=100`: the population launches take whole 16-row tiles only, so the sweep falls back to one train() per
  job (tests/test_sweep_config_cpu.py checks the grouping) - and each job must train to the end: checkpoints, finite scores, updates logged at the batch asked for."""
  import numpy as np
  import torch
  _bodies(monkeypatch)
  sys.path.insert(0, os.path.dirname(HERE))
  import train
  monkeypatch.chdir(tmp_path)
  root, scores = train.multirun(['-m', 'seed=3,4', 'algorithm=SAC', 'env=hopper', 'steps=50', 'training.start=40', 'evaluation.interval=25', 'evaluation.episodes=1', 'logging.interval=2',
                                 '+synthetic_env.max_episode_steps=20', '+synthetic_env.dataset_trajectories=6', 'training.batch_size=100', 'reinforcement.actor.hidden_size=64',
                                 'reinforcement.critic.hidden_size=64'], stamp='ragged')
  err = capsys.readouterr().err
  assert err.count('runs on its own, one job after another: training.batch_size=100 is not a multiple of 16') == 2
  assert len(scores) == 2 and np.isfinite(scores).all()
  actors = []
  for j in (0, 1):
    agent = torch.load(os.path.join(root, str(j), 'agent.pth'), weights_only=False)
    metrics = torch.load(os.path.join(root, str(j), 'metrics.pth'), weights_only=False)
    assert all(torch.isfinite(v).all() for v in agent['actor'].values()) and len(metrics['update_steps']) >= 2
    assert all(np.isfinite(q).all() and q.shape == (100,) for q in metrics['Q_values'])
    actors.append(agent['actor'])
  assert any(not torch.equal(v, actors[1][k]) for k, v in actors[0].items())   # two seeds, two learners
