"""The AdRIL / SQIL population relabel launch (il_batch_mix_relabel_population: k_mix_relabel_population), il.BatchedPopulationPlan('AdRIL') and the AdRIL seed sweep of
train.py on the host emulation of the kernels (tests/host_emu): the bodies of tests/test_population_adril_gpu.py with the library handle swapped for the emulation, as
tests/test_population_red_emulated.py runs its GPU bodies. The emulated lanes do not run in lockstep, a misaligned 16-byte lane traps here, and under IL_EMU_SCHEDULE the
workgroups of a launch run in a shuffled order (test_mix_relabel_population_does_not_depend_on_the_schedule)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402,F401
import test_population_acting_emulated as PA  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_population_adril_gpu.py (and the sweep helpers of tests/test_population_acting_gpu.py) with their GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tp = PA._bodies(monkeypatch)
  import test_population_adril_gpu as ta
  from imitation_learning_amd import memory as il_memory, training as il_training
  for k in ('DEV', 'N', 'T', 'Cfg', 'fill_memory'):
    monkeypatch.setattr(ta, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tp.il), ('_lib', _lib), ('il_memory', il_memory), ('il_training', il_training)):
    monkeypatch.setattr(ta, k, v, raising=False)
  return ta, tp


@pytest.mark.parametrize('mode', [(0, 0), (1, 0), (2, 1), (2, 3), (2, 1250)], ids=['label0-mix', 'label1-SQIL', 'label2-AdRIL-freq1', 'label2-AdRIL-freq3', 'label2-AdRIL-freq1250'])
@pytest.mark.parametrize('dims', [(11, 3), (18, 6), (40, 17)], ids=['hopper-S11-A3', 'halfcheetah-absorbing-S18-A6', 'wide-S40-A17'])
def test_mix_relabel_population_equals_il_batch_mix_relabel_dyn_per_learner_on_the_emulated_kernels(monkeypatch, dims, mode):
  _bodies(monkeypatch)[0].test_mix_relabel_population_equals_il_batch_mix_relabel_dyn_per_learner(dims, mode)


@pytest.mark.parametrize('mode', [(2, 1250), (1, 0)], ids=['label2-AdRIL', 'label1-SQIL'])
def test_mix_relabel_population_against_the_oracle_on_the_emulated_kernels(monkeypatch, mode):
  _bodies(monkeypatch)[0].test_mix_relabel_population_against_the_oracle(mode)


def test_mix_relabel_population_serves_rows_off_the_16_byte_grid_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_mix_relabel_population_serves_rows_off_the_16_byte_grid()


def test_mix_relabel_population_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_mix_relabel_population_refusals()


@pytest.mark.parametrize('how', ['eager', 'captured'])
@pytest.mark.parametrize('update_freq', [2, 0], ids=['AdRIL-freq2', 'SQIL'])
@pytest.mark.parametrize('balanced', [True, False], ids=['balanced', 'halves'])
def test_adril_population_plan_equals_plan_run_per_learner_on_the_emulated_kernels(monkeypatch, balanced, update_freq, how):
  _bodies(monkeypatch)[0].test_adril_population_plan_equals_plan_run_per_learner(balanced, update_freq, how)


def test_adril_population_plan_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_adril_population_plan_refusals()


KERNEL_LEVEL = 'mix_relabel_population_equals or against_the_oracle or off_the_16_byte_grid or mix_relabel_population_refusals'   # the 19 cases above that call the entry point directly


def test_mix_relabel_population_does_not_depend_on_the_schedule():
  """The kernel-level cases above with the lanes of every wave and the workgroups of every launch in a random order (IL_EMU_SCHEDULE is read once per process, hence the
  child): a learner's rows must not depend on which learner's workgroup runs first."""
  import subprocess
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k', KERNEL_LEVEL], env=dict(os.environ, IL_EMU_SCHEDULE='random:3'),
                     cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=1500)
  assert r.returncode == 0 and '19 passed' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_adril_seed_sweep_population_equals_per_learner_on_the_emulated_kernels(monkeypatch, tmp_path, capsys):
  """tests/test_population_adril_gpu.py::test_adril_seed_sweep_population_equals_per_learner[shipped-balanced], shortened: `-m seed=3,4 algorithm=AdRIL env=hopper
  +sweep.adril_population=true` under both schedules."""
  ta, tp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  ta.adril_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, [], PA.SHORT, tp, min_updates=1)
