"""PWIL through the acting worker and the device-resident expert relabel (il_pwil_act_reward, il_pwil_relabel_rows: k_pwil_couple; IL_ACT_REWARD_ON_DEVICE in k_act_step,
k_act_step_general and k_act_commit_general) on the host emulation of the kernels (tests/host_emu): the bodies of tests/test_pwil_acting_gpu.py with the library handle
swapped for the emulation, as tests/test_acting_general_emulated.py runs its GPU file. The emulator's lanes and workgroups do not run in lockstep and its graph replays
are real replays, which makes this the regression test for the gate of the merge (a coupling replayed without a new post must consume nothing; the overlap body also
posts between a replayed coupling and its append, which must then leave the post to the pair behind it), for the arrival ticket and for the reset inside the kernel
(under the overlap schedule a host-issued reset() would run ahead of the coupling it belongs behind)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402


def _bodies(monkeypatch):
  """tests/test_pwil_acting_gpu.py with its GPU-only names bound to the CPU and the emulated library."""
  import gpu_util
  tgp = E._emulated_product(monkeypatch, streams=True)
  import test_pwil_acting_gpu as tp
  for k in ('DEV', 'N', 'Cfg'):
    monkeypatch.setattr(tp, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tgp.il), ('_lib', _lib)):
    monkeypatch.setattr(tp, k, v, raising=False)
  return tp


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('schedule', ['exact', 'fused', 'overlap'])
def test_pwil_worker_matches_separate_calls_on_the_emulated_kernels(monkeypatch, schedule, absorbing):
  _bodies(monkeypatch).test_pwil_worker_matches_separate_calls(schedule, absorbing, 'n600_t40')


@pytest.mark.parametrize('shape', ['d3_tanh_h48_hopper', 'h50_d2_relu_hopper'])
def test_pwil_worker_with_a_general_actor_on_the_emulated_kernels(monkeypatch, shape):
  _bodies(monkeypatch).test_pwil_worker_with_a_general_actor(shape)


@pytest.mark.parametrize('horizon', [120, 170])
def test_pwil_relabel_memory_matches_the_row_loop_on_the_emulated_kernels(monkeypatch, horizon):
  _bodies(monkeypatch).test_pwil_relabel_memory_matches_the_row_loop(horizon)


@pytest.mark.parametrize('n,horizon,why', [(3000, 10, 'm > 256'), (6000, 30, 'G m > 4096')], ids=['one_workgroup_size', 'two_launch_size'])
def test_pwil_device_coupling_loud_failures_on_the_emulated_kernels(monkeypatch, n, horizon, why):
  _bodies(monkeypatch).test_pwil_device_coupling_loud_failures(n, horizon, why)


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
  score = train.train(config.compose(['algorithm=PWIL', 'env=walker2d'] + extra + SHORT))
  return score, torch.load(d / 'agent.pth', weights_only=False), torch.load(d / 'metrics.pth', weights_only=False)


def test_train_py_pwil_on_the_emulated_kernels(monkeypatch, tmp_path):
  """tests/test_pwil_acting_gpu.py's train.py runs, shortened: the default schedule (exact, the coupling launch in front of each append, no compute_reward and no reset()
  from the host) saves the learner of +acting.schedule=per_function, bit for bit, with equal train_returns; the overlap schedule (coupling and append as hooks of the
  PWIL plan) runs to the end."""
  import numpy as np
  import torch
  emulated = E._emulated_product(monkeypatch, streams=True)
  calls = []
  real = emulated.il.ActingWorker._launch
  monkeypatch.setattr(emulated.il.ActingWorker, '_launch', lambda self, *a, **k: (calls.append(self.reward_model is not None), real(self, *a, **k))[1])
  score_w, agent_w, metrics_w = _train(monkeypatch, tmp_path, 'worker', [])
  assert len(calls) >= 2 * 140 and all(calls)
  n = len(calls)
  score_p, agent_p, metrics_p = _train(monkeypatch, tmp_path, 'per_function', ['+acting.schedule=per_function'])
  assert len(calls) == n and np.isfinite(score_w) and score_w == score_p
  for part in ('actor', 'critic'):
    for k, v in agent_w[part].items():
      np.testing.assert_array_equal(v.numpy(), agent_p[part][k].numpy(), err_msg=f'{part}: {k}')
  np.testing.assert_array_equal(agent_w['log_alpha'].numpy(), agent_p['log_alpha'].numpy())
  assert metrics_w['train_returns'] == metrics_p['train_returns'] and len(metrics_w['train_returns']) >= 2
  for a, b in zip(metrics_w['predicted_rewards'], metrics_p['predicted_rewards']): np.testing.assert_array_equal(a, b)
  score_o, agent_o, metrics_o = _train(monkeypatch, tmp_path, 'overlap', ['+acting.schedule=overlap'])
  assert np.isfinite(score_o) and all(torch.isfinite(v).all() for v in agent_o['actor'].values())
  assert all(np.isfinite(r).all() and (r >= 0).all() for r in metrics_o['predicted_rewards'])
