"""Lockstep evaluation (il_act_eval_rows, il.LockstepEvaluator, evaluate_agent_lockstep / evaluate_population_lockstep, +evaluation.schedule=lockstep) on the host emulation
of the kernels (tests/host_emu): the bodies of tests/test_lockstep_eval_gpu.py with the library handle swapped for the emulation, as tests/test_mixed_population_emulated.py
binds its bodies. The emulator bounds-checks every LDS and global access, so this is the CPU-side check of what the launch sizes on the host - the LDS allocation (the widest
learner's; a launch sized for a narrower one would run the widest learner's layout off the end of it) - and of the mailbox layout (a row, an action or an echo outside
il_eval_mailbox_floats would be a store outside the block)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402,F401
import test_population_acting_emulated as PA  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402
import test_lockstep_eval_gpu as tle  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_lockstep_eval_gpu.py with its GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tp = PA._bodies(monkeypatch)
  for k in ('DEV', 'N', 'Cfg'):
    monkeypatch.setattr(tle, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tp.il), ('_lib', _lib)):
    monkeypatch.setattr(tle, k, v, raising=False)
  return tle, tp


@pytest.mark.parametrize('full', [True, False], ids=['max_rows=n', 'max_rows=48'])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 33])
@pytest.mark.parametrize('shape', tle.SHAPES, ids=['S11-A3-H64', 'S18-A6-H128', 'S112-A8-H256'])
def test_rows_equal_the_per_function_greedy_action_on_the_emulated_kernels(monkeypatch, shape, n, full):
  _bodies(monkeypatch)[0].test_rows_equal_the_per_function_greedy_action(shape, n, full)


def test_rows_of_a_state_wide_enough_for_the_lds_opt_in_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_rows_of_a_state_wide_enough_for_the_lds_opt_in()


@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_learners_of_different_widths_equal_their_single_learner_launches_on_the_emulated_kernels(monkeypatch, order):
  _bodies(monkeypatch)[0].test_learners_of_different_widths_equal_their_single_learner_launches(order)


def test_replayed_launch_second_post_and_sequence_wrap_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_replayed_launch_second_post_and_sequence_wrap()


def test_episodes_of_different_lengths_equal_evaluate_agent_per_environment_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_episodes_of_different_lengths_equal_evaluate_agent_per_environment()


def test_population_equals_evaluate_agent_lockstep_per_learner_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_population_equals_evaluate_agent_lockstep_per_learner()


def test_population_of_the_three_widths_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_population_of_the_three_widths()


def test_refusals_come_before_any_launch_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch)[0].test_refusals_come_before_any_launch()


def test_train_under_both_evaluation_schedules_on_the_emulated_kernels(monkeypatch, tmp_path):
  """`train.py algorithm=SAC env=halfcheetah seed=3`, shortened (tests/test_population_acting_emulated.py SHORT), under `sequential` and under `lockstep`."""
  t, _ = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  t.train_schedules_leave_the_same_agent(tmp_path, PA.SHORT)


def test_sweep_under_lockstep_evaluation_on_the_emulated_kernels(monkeypatch, tmp_path):
  """`-m seed=3,4 algorithm=SAC env=halfcheetah +evaluation.schedule=lockstep save_trajectories=true`, shortened, under both sweep schedules."""
  t, tp = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  t.sweep_schedules_leave_the_same_bytes_under_lockstep(tmp_path, PA.SHORT, tp)


def test_train_all_under_lockstep_evaluation_on_the_emulated_kernels(monkeypatch, tmp_path):
  """`train_all.py algorithm=SAC seed=3 +evaluation.schedule=lockstep save_trajectories=true`, shortened: four widths through one evaluator."""
  import test_mixed_population_emulated as MX
  t, _ = _bodies(monkeypatch)
  tmx = MX._bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  t.train_all_schedules_leave_the_same_bytes_under_lockstep(tmp_path, PA.SHORT, tmx)
