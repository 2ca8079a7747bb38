"""Lockstep evaluation for general actor shapes (il_act_eval_rows_general, il.GeneralLockstepEvaluator, evaluate_agent_lockstep with a general actor,
+evaluation.schedule=lockstep at a general actor shape) on the host emulation of the kernels (tests/host_emu): the bodies of tests/test_lockstep_eval_general_gpu.py with
the library handle swapped for the emulation, as tests/test_lockstep_eval_emulated.py binds its own. The emulator bounds-checks every LDS and global access, so this is the
CPU-side check of what the launch sizes on the host - the LDS allocation (gt_fwd_lds of the widest learner; a launch sized for a narrower one would run the widest
learner's layout off the end of it) - and of the mailbox layout (a row, an action or an echo outside il_eval_mailbox_floats would be a store outside the block).

No shape is left to the GPU alone: every case takes well under a minute here, the (512, 8, 512, 2, tanh) case included - the one whose LDS passes 64 KiB."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
import test_lockstep_eval_emulated as LE  # noqa: E402
import test_population_acting_emulated as PA  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402
import test_lockstep_eval_general_gpu as tlg  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_lockstep_eval_general_gpu.py (and tests/test_lockstep_eval_gpu.py, whose helpers it uses) with their GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tle, tp = LE._bodies(monkeypatch)
  for k in ('DEV', 'N', 'Cfg'):
    monkeypatch.setattr(tlg, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tp.il), ('_lib', _lib)):
    monkeypatch.setattr(tlg, k, v, raising=False)
  monkeypatch.setattr(tlg, '_library_path', lambda: E.emu()._name)   # the IL_GENERAL_TILES=0 refusal, decided in a process of its own: by the emulated library's host code
  return tlg


@pytest.mark.parametrize('full', [True, False], ids=['max_rows=n', 'max_rows=48'])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 33])
@pytest.mark.parametrize('shape', tlg.SHAPES, ids=tlg.SHAPE_IDS)
def test_rows_equal_the_per_function_greedy_action_on_the_emulated_kernels(monkeypatch, shape, n, full):
  _bodies(monkeypatch).rows_equal_the_per_function_greedy_action(shape, n, full)


def test_rows_of_the_widest_shape_take_the_lds_opt_in_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_rows_of_the_widest_shape_take_the_lds_opt_in()


@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_learners_of_different_widths_equal_their_single_learner_launches_on_the_emulated_kernels(monkeypatch, order):
  _bodies(monkeypatch).test_learners_of_different_widths_equal_their_single_learner_launches(order)


def test_replayed_launch_second_post_and_sequence_wrap_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_replayed_launch_second_post_and_sequence_wrap()


def test_refusals_come_before_any_launch_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_refusals_come_before_any_launch()


def test_episodes_of_different_lengths_equal_evaluate_agent_per_environment_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_episodes_of_different_lengths_equal_evaluate_agent_per_environment()


def test_train_with_a_general_actor_under_both_evaluation_schedules_on_the_emulated_kernels(monkeypatch, tmp_path):
  """`train.py algorithm=SAC env=halfcheetah seed=3` with a depth-3 tanh hidden-48 actor, shortened (tests/test_population_acting_emulated.py SHORT), under `sequential`
  and under `lockstep`."""
  t = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  t.train_schedules_leave_the_same_agent(tmp_path, PA.SHORT)
