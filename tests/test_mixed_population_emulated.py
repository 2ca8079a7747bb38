"""Populations of learners of different state / action widths (il_sac_update_population_mixed, il_act_step_population_mixed, il_gail_step_population_mixed) on the host
emulation of the kernels (tests/host_emu): the bodies of tests/test_mixed_population_gpu.py with the library handle swapped for the emulation, as
tests/test_population_acting_emulated.py binds its bodies. The emulator bounds-checks every LDS and global access, so this is the CPU-side check of what the mixed launches
size on the host: the tile kernels' LDS allocation (the widest learner's; a launch sized from the narrowest learner's descriptor would run the widest learner's layout off
the end of it), the optimiser launches' grids (a narrower learner's surplus workgroups must end before they touch anything) and the per-learner mailbox layout."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402,F401
import test_population_acting_emulated as PA  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402
import test_mixed_population_gpu as tmx  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_mixed_population_gpu.py (and the helpers of tests/test_population_acting_gpu.py it drives) with their GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tp = PA._bodies(monkeypatch)
  from imitation_learning_amd import memory as il_memory, training as il_training
  for k in ('DEV', 'N', 'T', 'Cfg', 'fill_memory'):
    monkeypatch.setattr(tmx, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tp.il), ('_lib', _lib), ('il_memory', il_memory), ('il_training', il_training), ('tp', tp)):
    monkeypatch.setattr(tmx, k, v, raising=False)
  return tmx


@pytest.mark.parametrize('order', list(tmx.ORDERS))
@pytest.mark.parametrize('B,H', [(64, 64), (48, 64), (64, 128)], ids=['B64-H64-blocks', 'B48-H64-tiles', 'B64-H128-blocks'])
def test_mixed_sac_population_equals_plan_run_per_learner_on_the_emulated_kernels(monkeypatch, B, H, order):
  _bodies(monkeypatch).test_mixed_sac_population_equals_plan_run_per_learner(B, H, order)


@pytest.mark.parametrize('B', [64, 48])
def test_uniform_population_of_each_width_gives_the_mixed_population_s_bytes_on_the_emulated_kernels(monkeypatch, B):
  _bodies(monkeypatch).test_uniform_population_of_each_width_gives_the_mixed_population_s_bytes(B)


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
@pytest.mark.parametrize('H', [64, 128])
def test_mixed_population_acting_matches_per_learner_workers_on_the_emulated_kernels(monkeypatch, H, schedule, absorbing):
  _bodies(monkeypatch).test_mixed_population_acting_matches_per_learner_workers(H, schedule, absorbing)


@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_mixed_population_acting_idle_learner_on_the_emulated_kernels(monkeypatch, schedule):
  _bodies(monkeypatch).test_mixed_population_acting_idle_learner(schedule)


def test_mixed_evaluate_population_equals_evaluate_agent_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_mixed_evaluate_population_equals_evaluate_agent()


@pytest.mark.parametrize('widths', [tmx.W, tmx.W[::-1]], ids=['narrowest-first', 'widest-first'])
@pytest.mark.parametrize('loss', ['BCE', 'PUGAIL'])
def test_mixed_gail_step_population_equals_the_per_learner_sequence_on_the_emulated_kernels(monkeypatch, loss, widths):
  _bodies(monkeypatch).test_mixed_gail_step_population_equals_the_per_learner_sequence(loss, widths)


@pytest.mark.parametrize('loss', ['BCE', 'PUGAIL'])
def test_mixed_gail_population_plan_equals_plan_run_per_learner_on_the_emulated_kernels(monkeypatch, loss):
  _bodies(monkeypatch).test_mixed_gail_population_plan_equals_plan_run_per_learner(loss)


def test_mixed_population_plan_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_mixed_population_plan_refusals()


def test_mixed_widths_with_other_algorithms_are_refused_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_mixed_widths_with_other_algorithms_are_refused()


def test_mixed_acting_worker_refusals_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_mixed_acting_worker_refusals()


def test_mixed_entry_points_refuse_bad_arguments_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_mixed_entry_points_refuse_bad_arguments()


def test_replay_sample_population_serves_rows_of_different_widths_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_replay_sample_population_serves_rows_of_different_widths()


@pytest.mark.parametrize('algorithm', ['SAC', 'GAIL'])
def test_train_all_population_equals_per_learner_on_the_emulated_kernels(monkeypatch, tmp_path, algorithm):
  """`train_all.py algorithm=<ALG> seed=3`, shortened (tests/test_population_acting_emulated.py SHORT), under both schedules."""
  t = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  t.train_all_schedules_leave_the_same_bytes(tmp_path, algorithm, PA.SHORT, min_updates=1)


def test_train_all_graph_replays_equal_direct_launches_on_the_emulated_kernels(monkeypatch, tmp_path):
  t = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  t.test_train_all_graph_replays_equal_direct_launches(tmp_path, monkeypatch, short=PA.SHORT)


def test_train_all_multirun_of_two_seeds_is_one_population_of_eight_on_the_emulated_kernels(monkeypatch, tmp_path, capsys):
  t = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  t.test_train_all_multirun_of_two_seeds_is_one_population_of_eight(tmp_path, capsys, short=PA.SHORT)


def test_train_all_without_mixed_population_launches_on_the_emulated_kernels(monkeypatch, tmp_path, capsys):
  t = _bodies(monkeypatch)
  monkeypatch.chdir(tmp_path)
  t.test_train_all_without_mixed_population_launches_trains_environment_after_environment(tmp_path, capsys, short=PA.SHORT)
