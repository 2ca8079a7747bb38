"""The GMMIL population reward launch (il_gmmil_reward_population: k_gmmil_mfma_pop), il.BatchedPopulationPlan('GMMIL') and the GMMIL seed sweep of train.py on the host
emulation of the kernels (tests/host_emu): the bodies of tests/test_population_gmmil_gpu.py with the library handle swapped for the emulation, as
tests/test_population_red_emulated.py runs RED's. Under IL_EMU_SCHEDULE the waves of a workgroup and the workgroups of a launch run in a shuffled order
(test_gmmil_reward_population_does_not_depend_on_the_schedule): whichever learner's workgroup arrives first, a learner's last arriver counts that learner's tickets only."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402,F401
import test_population_acting_emulated as PA  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_population_gmmil_gpu.py (and the sweep helpers of tests/test_population_acting_gpu.py) with their GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tp = PA._bodies(monkeypatch)
  import test_population_gmmil_gpu as tg
  from imitation_learning_amd import training as il_training
  for k in ('DEV', 'N', 'T', 'Cfg', 'fill_memory'):
    monkeypatch.setattr(tg, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tp.il), ('_lib', _lib), ('il_training', il_training)):
    monkeypatch.setattr(tg, k, v, raising=False)
  return tg, tp


@pytest.mark.parametrize('case', ['SHIPPED', 'HOPPER', 'RAGGED', 'NKQ4_EDGE', 'ANT', 'LIMIT', 'NINE_LEARNERS', 'SHIPPED_STATE_ONLY'])
def test_gmmil_reward_population_equals_il_gmmil_reward_per_learner_on_the_emulated_kernels(monkeypatch, case):
  tg, _ = _bodies(monkeypatch)
  tg.test_gmmil_reward_population_equals_il_gmmil_reward_per_learner(getattr(tg, case))


def test_gmmil_reward_population_whole_lanes_promise_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_gmmil_reward_population_whole_lanes_is_a_promise_about_requests_not_values()


def test_gmmil_reward_population_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_gmmil_reward_population_refusals()


def mfma_off_child():
  """What the child process of the next test runs (IL_GMMIL_MFMA=0 is read once per process)."""
  mp = pytest.MonkeyPatch()
  try:
    _bodies(mp)[0].mfma_off_body()
  finally:
    mp.undo()


MFMA_OFF_CHILD = 'import sys; sys.path[:0] = [{root!r}, {root!r} + "/tests", {root!r} + "/tests/golden"]; import test_population_gmmil_emulated as t; t.mfma_off_child()'


def test_gmmil_reward_population_is_unsupported_under_IL_GMMIL_MFMA_0_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_gmmil_reward_population_is_unsupported_under_IL_GMMIL_MFMA_0(child=MFMA_OFF_CHILD)


@pytest.mark.parametrize('how', ['overlap', 'in stream order', 'captured'])
def test_gmmil_population_plan_equals_plan_run_per_learner_on_the_emulated_kernels(monkeypatch, how):
  _bodies(monkeypatch)[0].test_gmmil_population_plan_equals_plan_run_per_learner(monkeypatch, how)


def test_gmmil_population_plan_refuses_mismatched_learners_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_gmmil_population_plan_refuses_mismatched_learners()


KERNEL_LEVEL = 'gmmil_reward_population_equals or whole_lanes or refusals'   # the 10 cases above that call the entry point directly in this process


def test_gmmil_reward_population_does_not_depend_on_the_schedule():
  """The kernel-level cases above with the waves of every workgroup, the lanes of every wave and the workgroups of every launch in a random order (IL_EMU_SCHEDULE is read
  once per process, hence the child): a learner's rewards must not depend on which learner's workgroup arrives first."""
  import subprocess
  r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k', KERNEL_LEVEL], env=dict(os.environ, IL_EMU_SCHEDULE='random:3'),
                     cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=1500)
  assert r.returncode == 0 and '10 passed' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_gmmil_seed_sweep_population_equals_per_learner_on_the_emulated_kernels(monkeypatch, tmp_path, capsys):
  """tests/test_population_gmmil_gpu.py::test_gmmil_seed_sweep_population_equals_per_learner[shipped], shortened: `-m seed=3,4 algorithm=GMMIL env=hopper` under both schedules."""
  tg, tp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  tg.gmmil_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, [], PA.SHORT, tp, min_updates=1)
