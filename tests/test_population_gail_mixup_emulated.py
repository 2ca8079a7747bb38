"""The Mixup population discriminator step (il_gail_mixup_step_population: k_gail_mix_fill_pop, k_gail_grad_pop with the learners' il_gail_extra array),
il.BatchedPopulationPlan of Mixup learners and the Mixup seed sweep of train.py on the host emulation of the kernels (tests/host_emu): the bodies of
tests/test_population_gail_mixup_gpu.py with the library handle swapped for the emulation, as tests/test_population_adril_emulated.py runs its GPU bodies. The emulated
lanes do not run in lockstep - a coefficient read from a place the loss section of another lane of the row writes would show here - and under IL_EMU_SCHEDULE the lanes of
every wave and the workgroups of a launch run in a shuffled order (test_mixup_step_population_does_not_depend_on_the_schedule)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402,F401
import test_population_acting_emulated as PA  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402
import test_population_gail_mixup_gpu as tm  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_population_gail_mixup_gpu.py (and the sweep helpers of tests/test_population_acting_gpu.py) with their GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tp = PA._bodies(monkeypatch)
  from imitation_learning_amd import memory as il_memory, training as il_training
  for k in ('DEV', 'N', 'T', 'Cfg', 'close_params', 'fill_memory'):
    monkeypatch.setattr(tm, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tp.il), ('_lib', _lib), ('il_memory', il_memory), ('il_training', il_training)):
    monkeypatch.setattr(tm, k, v, raising=False)
  return tm, tp


@pytest.mark.parametrize('c', [pytest.param(c, id=tm._case_id(c)) for c in tm.CASES])
def test_mixup_step_population_equals_the_per_learner_sequence_on_the_emulated_kernels(monkeypatch, c):
  _bodies(monkeypatch)[0].test_mixup_step_population_equals_the_per_learner_sequence(c)


@pytest.mark.parametrize('alpha', [1.0, 0.4])
def test_mixup_step_population_against_the_oracle_on_the_emulated_kernels(monkeypatch, alpha):
  _bodies(monkeypatch)[0].test_mixup_step_population_against_the_oracle(alpha)


def test_mixup_step_population_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_mixup_step_population_refusals()


@pytest.mark.parametrize('how', ['eager', 'captured'])
@pytest.mark.parametrize('alpha', [1.0, 0.4])
def test_mixup_population_plan_equals_plan_run_per_learner_on_the_emulated_kernels(monkeypatch, alpha, how):
  _bodies(monkeypatch)[0].mixup_population_plan_equals_plan_run_per_learner(alpha, how, side=True)


@pytest.mark.parametrize('how', ['eager', 'captured'])
@pytest.mark.parametrize('alpha', [1.0, 0.4])
def test_mixup_population_plan_on_one_stream_on_the_emulated_kernels(monkeypatch, alpha, how):
  monkeypatch.setenv('IL_POP_OVERLAP', '0')
  _bodies(monkeypatch)[0].mixup_population_plan_equals_plan_run_per_learner(alpha, how, side=False)


def test_mixup_population_plan_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_mixup_population_plan_refusals()


KERNEL_LEVEL = 'equals_the_per_learner_sequence or against_the_oracle or step_population_refusals'   # the cases above that call the entry point directly
N_KERNEL_LEVEL = len(tm.CASES) + 3


def test_mixup_step_population_does_not_depend_on_the_schedule():
  """The kernel-level cases above with the lanes of every wave and the workgroups of every launch in a random order (IL_EMU_SCHEDULE is read once per process, hence the
  child): a learner's result must not depend on which learner's workgroup runs first, nor on the order of the lanes inside a row - the 16 lanes of a row read the row's
  coefficient while one of them stores the row's logit."""
  import subprocess
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k', KERNEL_LEVEL], env=dict(os.environ, IL_EMU_SCHEDULE='random:3'),
                     cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=1500)
  assert r.returncode == 0 and f'{N_KERNEL_LEVEL} passed' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize('extra', [[], ['imitation.mixup_alpha=0.5'], tm.GAIL_10_DISC], ids=['alpha1', 'alpha0.5', 'GAIL_10-discriminator-no-spectral-norm'])
def test_mixup_seed_sweep_population_equals_per_learner_equals_single_runs_on_the_emulated_kernels(monkeypatch, tmp_path, capsys, extra):
  """tests/test_population_gail_mixup_gpu.py's sweep, shortened: `-m seed=3,4 algorithm=GAIL env=hopper imitation.loss_function=Mixup +sweep.gail_mixup_population=true`
  under both schedules and as two single train() runs."""
  tmx, tp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  tmx.mixup_sweep_schedules_and_single_runs_leave_the_same_bytes(tmp_path, capsys, extra, PA.SHORT, tp, min_updates=1)
