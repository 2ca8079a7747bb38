"""The acting worker for general actor shapes (il_act_step_general: k_act_step_general, k_act_commit_general) on the host emulation of the kernels (tests/host_emu): the
bodies of tests/test_acting_general_gpu.py with the library handle swapped for the emulation, as tests/test_kernels_host_emulation.py runs the other `-m gpu` bodies.
The emulator's lanes do not run in lockstep, so the rows-wider-than-the-workgroup cases are the regression test for the strided append and for the cursor store
behind the last barrier. The depth-8 hidden-512 shape stays GPU-only (about 7 MB of weights per step through the emulated MFMAs: minutes here, nothing the smaller
form-(a) shapes do not already run)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_acting_general_gpu.py with its GPU-only names bound to the CPU and the emulated library (and test_timed_path_oracle's, for record_noise)."""
  import gpu_util
  tgp = E._emulated_product(monkeypatch, streams=True)
  E._timed_path_modules(monkeypatch, tgp)
  import test_acting_general_gpu as tg
  for k in ('DEV', 'N', 'Cfg', 'close'):
    monkeypatch.setattr(tg, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tgp.il), ('_lib', _lib)):
    monkeypatch.setattr(tg, k, v, raising=False)
  return tg


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('shape,schedule', [('d3_tanh_h48_hopper', 'exact'), ('d3_tanh_h48_hopper', 'fused'), ('d3_tanh_h48_hopper', 'overlap'), ('d1_sigmoid_h80_halfcheetah', 'fused'),
                                            ('wide_h128_d2', 'exact'), ('wide_h128_d2', 'fused'), ('h50_d2_relu_hopper', 'exact'), ('h50_d2_relu_hopper', 'fused')])
def test_general_acting_worker_matches_separate_calls_on_the_emulated_kernels(monkeypatch, shape, absorbing, schedule):
  _bodies(monkeypatch).test_general_acting_worker_matches_separate_calls(shape, absorbing, schedule)


@pytest.mark.parametrize('schedule', ['exact', 'fused'])
@pytest.mark.parametrize('shape', ['d3_tanh_h48_hopper', 'd1_sigmoid_h80_halfcheetah', 'wide_h128_d2', 'h50_d2_relu_hopper'])
def test_general_acting_replays_through_the_oracle_on_the_emulated_kernels(monkeypatch, shape, schedule):
  _bodies(monkeypatch).test_general_acting_replays_through_the_oracle(shape, schedule)


@pytest.mark.parametrize('S,A,H,depth,activation,absorbing', [(300, 4, 64, 2, 'tanh', True), (300, 4, 64, 2, 'tanh', False), (512, 8, 16, 1, 'relu', True)],
                         ids=['row609_absorbing', 'row609_plain', 'row1037_h16'])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_general_acting_rows_wider_than_the_workgroup_on_the_emulated_kernels(monkeypatch, S, A, H, depth, activation, absorbing, schedule):
  _bodies(monkeypatch).test_general_acting_rows_wider_than_the_workgroup(S, A, H, depth, activation, absorbing, schedule)


@pytest.mark.parametrize('shape', ['d3_tanh_h48_hopper', 'wide_h128_d2'])
def test_general_acting_greedy_on_the_emulated_kernels(monkeypatch, shape):
  _bodies(monkeypatch).test_general_acting_greedy(shape)


def test_general_acting_mirror_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_general_acting_mirror_serves_the_published_parameters()


def test_general_acting_loud_failures_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_general_acting_loud_failures()


SHORT = ['steps=140', 'training.start=120', 'evaluation.interval=70', 'evaluation.episodes=1', 'logging.interval=10', '+synthetic_env.max_episode_steps=60', '+synthetic_env.dataset_trajectories=6',
         'training.batch_size=64']   # (the shortened run of test_train_py_end_to_end_on_the_emulated_kernels)


def _train(monkeypatch, tmp_path, name, extra):
  import torch
  sys.path.insert(0, os.path.dirname(HERE))
  import train
  from imitation_learning_amd import config
  from imitation_learning_amd import training as il_training
  il_training._NOISE.clear(); il_training._WS.clear()   # the update noise counter lives with the process: every run starts from zero, like a fresh `python train.py`
  d = tmp_path / name
  d.mkdir()
  monkeypatch.chdir(d)
  score = train.train(config.compose(['algorithm=SAC', 'env=hopper', 'reinforcement.actor.depth=3', 'reinforcement.actor.activation=tanh', 'reinforcement.actor.hidden_size=48'] + extra + SHORT))
  return score, torch.load(d / 'agent.pth', weights_only=False)


def test_train_py_with_a_general_actor_on_the_emulated_kernels(monkeypatch, tmp_path):
  """tests/test_train_general_acting_gpu.py, shortened: train.py's default schedule (exact, through il_act_step_general) saves the learner of +acting.schedule=per_function,
  bit for bit; the overlap schedule (append and parameter snapshot as hooks of the general-shape plan) runs to the end."""
  import numpy as np
  import torch
  _emulated = E._emulated_product(monkeypatch, streams=True)
  calls = []
  real = _emulated.il.ActingWorker._launch
  monkeypatch.setattr(_emulated.il.ActingWorker, '_launch', lambda self, *a, **k: (calls.append(self.general and self.one_launch), real(self, *a, **k))[1])
  score_w, agent_w = _train(monkeypatch, tmp_path, 'worker', [])
  assert len(calls) >= 2 * 140 and all(calls)
  n = len(calls)
  score_p, agent_p = _train(monkeypatch, tmp_path, 'per_function', ['+acting.schedule=per_function'])
  assert len(calls) == n and np.isfinite(score_w) and score_w == score_p
  for part in ('actor', 'critic'):
    for k, v in agent_w[part].items():
      np.testing.assert_array_equal(v.numpy(), agent_p[part][k].numpy(), err_msg=f'{part}: {k}')
  np.testing.assert_array_equal(agent_w['log_alpha'].numpy(), agent_p['log_alpha'].numpy())
  score_o, agent_o = _train(monkeypatch, tmp_path, 'overlap', ['+acting.schedule=overlap'])
  assert np.isfinite(score_o) and all(torch.isfinite(v).all() for v in agent_o['actor'].values())
