"""The RED population reward launch (il_red_reward_population: k_red_eval_population), il.BatchedPopulationPlan('RED') and the RED seed sweep of train.py on the host
emulation of the kernels (tests/host_emu): the bodies of tests/test_population_red_gpu.py with the library handle swapped for the emulation, as
tests/test_population_acting_emulated.py runs its GPU bodies. The emulated workgroup's LDS is allocated to the byte and its lanes do not run in lockstep; under
IL_EMU_SCHEDULE the waves of a workgroup and the workgroups of a launch run in a shuffled order (test_red_reward_population_does_not_depend_on_the_schedule)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
import test_population_acting_emulated as PA  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_population_red_gpu.py (and the sweep helpers of tests/test_population_acting_gpu.py) with their GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tp = PA._bodies(monkeypatch)
  import test_population_red_gpu as tr
  from imitation_learning_amd import training as il_training
  for k in ('DEV', 'N', 'T', 'Cfg', 'fill_memory'):
    monkeypatch.setattr(tr, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tp.il), ('_lib', _lib), ('il_training', il_training)):
    monkeypatch.setattr(tr, k, v, raising=False)
  return tr, tp


@pytest.mark.parametrize('case', ['SHIPPED', 'RED_25', 'STATE_ONLY', 'LIMIT'])
def test_red_reward_population_equals_il_red_forward_per_learner_on_the_emulated_kernels(monkeypatch, case):
  tr, _ = _bodies(monkeypatch)
  tr.test_red_reward_population_equals_il_red_forward_per_learner(getattr(tr, case))


def test_red_reward_population_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_red_reward_population_refusals()


@pytest.mark.parametrize('how', ['overlap', 'in stream order', 'captured'])
def test_red_population_plan_equals_plan_run_per_learner_on_the_emulated_kernels(monkeypatch, how):
  _bodies(monkeypatch)[0].test_red_population_plan_equals_plan_run_per_learner(monkeypatch, how)


def test_red_population_plan_refuses_mismatched_discriminators_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_red_population_plan_refuses_mismatched_discriminators()


KERNEL_LEVEL = 'red_reward_population_equals or refusals'   # the 5 cases above that call the entry point directly


def test_red_reward_population_does_not_depend_on_the_schedule():
  """The kernel-level cases above with the waves of every workgroup, the lanes of every wave and the workgroups of every launch in a random order (IL_EMU_SCHEDULE is read
  once per process, hence the child): a learner's rewards must not depend on which learner's workgroup runs first."""
  import subprocess
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k', KERNEL_LEVEL], env=dict(os.environ, IL_EMU_SCHEDULE='random:3'),
                     cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=1500)
  assert r.returncode == 0 and '5 passed' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_red_seed_sweep_population_equals_per_learner_on_the_emulated_kernels(monkeypatch, tmp_path, capsys):
  """tests/test_population_red_gpu.py::test_red_seed_sweep_population_equals_per_learner[shipped], shortened: `-m seed=3,4 algorithm=RED env=hopper` under both schedules."""
  tr, tp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  tr.red_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, [], PA.SHORT, tp, min_updates=1)
