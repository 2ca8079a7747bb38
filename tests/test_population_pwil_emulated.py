"""PWIL seed sweeps as one population (il_pwil_act_reward_population: k_pwil_couple_population in front of k_act_step_population; il.PopulationActingWorker(reward_models=...))
on the host emulation of the kernels (tests/host_emu): the bodies of tests/test_population_pwil_gpu.py with the library handle swapped for the emulation, as
tests/test_pwil_acting_emulated.py runs its GPU file. The emulator's lanes and workgroups do not run in lockstep, which makes this the regression test for the per-learner
arrival count (a row of the grid narrower than the grid: its surplus workgroups must not take the learner's ticket), for the gate of the merge under replayed and idle
posts, and for the reset inside the kernel while the other learners are mid-episode."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_population_pwil_gpu.py, and the two GPU files whose helpers it uses, with their GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tgp = E._emulated_product(monkeypatch, streams=True)
  import test_population_acting_gpu as tpa
  import test_population_pwil_gpu as tpp
  import test_pwil_acting_gpu as tpw
  for mod in (tpp, tpa, tpw):
    for k in ('DEV', 'N', 'Cfg'):
      monkeypatch.setattr(mod, k, getattr(gpu_util, k), raising=False)
    for k, v in (('il', tgp.il), ('_lib', _lib)):
      monkeypatch.setattr(mod, k, v, raising=False)
  return tpp


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
@pytest.mark.parametrize('env', ['hopper', 'halfcheetah'])
def test_population_pwil_matches_per_learner_workers_on_the_emulated_kernels(monkeypatch, env, schedule, absorbing):
  _bodies(monkeypatch).test_population_pwil_matches_per_learner_workers(env, schedule, absorbing)


@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_population_pwil_idle_and_replayed_launches_change_nothing_on_the_emulated_kernels(monkeypatch, schedule):
  _bodies(monkeypatch).test_population_pwil_idle_and_replayed_launches_change_nothing(schedule)


def test_population_pwil_uncoupled_post_is_left_alone_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_population_pwil_uncoupled_post_is_left_alone()


def test_population_pwil_learner_wider_than_the_grid_is_not_coupled_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_population_pwil_learner_wider_than_the_grid_is_not_coupled()


def test_population_pwil_loud_failures_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_population_pwil_loud_failures()


KERNEL_LEVEL = 'population_pwil_matches or idle_and_replayed or uncoupled_post or wider_than_the_grid'   # the 12 cases above that launch the kernels


def test_population_pwil_does_not_depend_on_the_schedule():
  """The kernel-level cases above with the waves of every workgroup, the lanes of every wave and the workgroups of every launch in a random order (IL_EMU_SCHEDULE is read
  once per process, hence the child): which workgroup of a learner's row arrives last, and whether a surplus workgroup of a narrower row runs before or after it, must not
  show in any learner's rewards, weights, carry or ticket."""
  import subprocess
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k', KERNEL_LEVEL], env=dict(os.environ, IL_EMU_SCHEDULE='random:3'),
                     cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=1500)
  assert r.returncode == 0 and '12 passed' in r.stdout, (r.stdout + r.stderr)[-3000:]


SHORT = ['steps=140', 'training.start=120', 'evaluation.interval=70', 'evaluation.episodes=1', 'logging.interval=10', '+synthetic_env.max_episode_steps=60', '+synthetic_env.dataset_trajectories=6',
         'training.batch_size=64',   # (tests/test_pwil_acting_emulated.py SHORT)
         'reinforcement.actor.hidden_size=64', 'reinforcement.critic.hidden_size=64']   # the smallest fused shape: the emulated MFMAs are what these runs spend their time in


@pytest.mark.parametrize('extra', [[], ['imitation.mix_expert_data=prefill_memory']], ids=['none', 'prefill_memory'])
def test_pwil_seed_sweep_population_equals_per_learner_equals_single_runs_on_the_emulated_kernels(monkeypatch, tmp_path, capsys, extra):
  """tests/test_population_pwil_gpu.py's sweep, shortened: both sweep schedules and two single train() runs leave the same learners and metrics."""
  tpp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  tpp.test_pwil_seed_sweep_population_equals_per_learner_equals_single_runs(tmp_path, capsys, extra, short=SHORT)
