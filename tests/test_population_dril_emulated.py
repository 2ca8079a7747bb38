"""The DRIL population reward launch (il_dril_reward_population: k_dril_unc_population), the population BC auxiliary launch (il_bc_step_population),
il.BatchedPopulationPlan('DRIL') and the DRIL seed sweep of train.py on the host emulation of the kernels (tests/host_emu): the bodies of tests/test_population_dril_gpu.py
with the library handle swapped for the emulation, as tests/test_population_red_emulated.py runs its GPU bodies. The emulated workgroup's LDS is allocated to the byte and
its lanes do not run in lockstep; under IL_EMU_SCHEDULE the waves of a workgroup and the workgroups of a launch run in a shuffled order
(test_dril_population_launches_do_not_depend_on_the_schedule)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
import test_population_acting_emulated as PA  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_population_dril_gpu.py (and the sweep helpers of tests/test_population_acting_gpu.py) with their GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tp = PA._bodies(monkeypatch)
  import test_population_dril_gpu as td
  from imitation_learning_amd import training as il_training
  for k in ('DEV', 'N', 'T', 'Cfg', 'fill_memory'):
    monkeypatch.setattr(td, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tp.il), ('_lib', _lib), ('il_training', il_training)):
    monkeypatch.setattr(td, k, v, raising=False)
  return td, tp


@pytest.mark.parametrize('case', ['SHIPPED', 'DRIL_25', 'NO_DROPOUT', 'LIMIT'])
def test_dril_reward_population_equals_il_dril_uncertainty_per_learner_on_the_emulated_kernels(monkeypatch, case):
  td, _ = _bodies(monkeypatch)
  td.test_dril_reward_population_equals_il_dril_uncertainty_per_learner(getattr(td, case))


def test_dril_reward_population_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_dril_reward_population_refusals()


@pytest.mark.parametrize('shape', [(11, 3, 256, 32, 3), (17, 6, 128, 48, 2), (112, 8, 64, 16, 1)], ids=['hopper-H256-B32-L3', 'S17-A6-H128-B48-L2', 'S112-A8-H64-one-tile-one-learner'])
def test_bc_step_population_equals_il_bc_step_per_learner_on_the_emulated_kernels(monkeypatch, shape):
  _bodies(monkeypatch)[0].test_bc_step_population_equals_il_bc_step_per_learner(shape)


def test_bc_step_population_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_bc_step_population_refusals()


@pytest.mark.parametrize('bc_aux', [True, False], ids=['bc_aux', 'no-bc_aux'])
@pytest.mark.parametrize('how', ['overlap', 'in stream order', 'captured'])
def test_dril_population_plan_equals_plan_run_per_learner_on_the_emulated_kernels(monkeypatch, how, bc_aux):
  _bodies(monkeypatch)[0].test_dril_population_plan_equals_plan_run_per_learner(monkeypatch, how, bc_aux)


def test_dril_population_plan_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_dril_population_plan_refusals()


KERNEL_LEVEL = 'reward_population or bc_step_population'   # the 9 cases above that call the two entry points directly


def test_dril_population_launches_do_not_depend_on_the_schedule():
  """The kernel-level cases above with the waves of every workgroup, the lanes of every wave and the workgroups of every launch in a random order (IL_EMU_SCHEDULE is read
  once per process, hence the child): a learner's rewards, parameters and moments must not depend on which learner's workgroup runs first."""
  import subprocess
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k', KERNEL_LEVEL], env=dict(os.environ, IL_EMU_SCHEDULE='random:3'),
                     cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=1500)
  assert r.returncode == 0 and '9 passed' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize('extra', [[], ['imitation.bc_aux_loss=false', 'imitation.mix_expert_data=prefill_memory']], ids=['shipped-bc_aux', 'no-bc_aux-prefill'])
def test_dril_seed_sweep_population_equals_per_learner_on_the_emulated_kernels(monkeypatch, tmp_path, capsys, extra):
  """tests/test_population_dril_gpu.py::test_dril_seed_sweep_population_equals_per_learner, shortened: `-m seed=3,4 algorithm=DRIL env=hopper` under both schedules."""
  td, tp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  td.dril_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, PA.SHORT, tp, min_updates=1, iterations=8)
