"""Device-resident expert epochs (`il.PretrainPlan`, the *_epoch_steps entry points) on the host emulation of the kernels (tests/host_emu): the bodies of
tests/test_pretrain_plan_gpu.py with the library handle swapped for the emulation, as tests/test_acting_general_emulated.py wraps its GPU file - so the bit-for-bit
equality of the plan and the per-function loop, the split runs and the refusals are checked on a machine without a GPU too. The emulator's lanes do not run in lockstep:
the padded-tile cases are also the regression test for rows >= n reading the order table (the sanitised build bounds-checks it). The reference anchor (hidden 256, batch
256, 60 iterations through the emulated MFMAs) stays GPU-only."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402
import test_pretrain_plan_gpu as tg  # noqa: E402


class _Event:   # torch.cuda.Event: the emulated null stream runs every copy at once
  def record(self, *a, **k): pass
  def synchronize(self): pass


def _bodies(monkeypatch):
  import torch
  import gpu_util
  from imitation_learning_amd import memory as il_memory
  tgp = E._emulated_product(monkeypatch, streams=True)
  monkeypatch.setattr(torch.cuda, 'Event', _Event)
  for k in ('DEV', 'N', 'T', 'Cfg', 'close', 'close_params'):
    monkeypatch.setattr(tg, k, getattr(gpu_util, k), raising=False)
  for k, v in (('il', tgp.il), ('_lib', _lib), ('il_memory', il_memory)):
    monkeypatch.setattr(tg, k, v, raising=False)
  return tg


@pytest.mark.parametrize('case', list(tg.CASES))
def test_plan_equals_the_per_function_loop_on_the_emulated_kernels(monkeypatch, case):
  _bodies(monkeypatch).test_plan_equals_the_per_function_loop_bit_for_bit(case)


@pytest.mark.parametrize('case', ['bc_fused_b32', 'bc_tiles_d3_tanh_h48_b24', 'bc_layers_d2_relu_h50_b24', 'dril_d2_relu_h32_b20', 'red_d2_tanh_h64_drop_b20'])
def test_split_runs_equal_one_run_on_the_emulated_kernels(monkeypatch, case):
  _bodies(monkeypatch).test_split_runs_equal_one_run(case)


def test_loud_failures_on_the_emulated_kernels(monkeypatch):
  _bodies(monkeypatch).test_loud_failures()


SHORT = ['steps=140', 'training.start=120', 'evaluation.interval=70', 'evaluation.episodes=1', 'logging.interval=10', '+synthetic_env.max_episode_steps=60', '+synthetic_env.dataset_trajectories=6',
         'training.batch_size=64']   # (the shortened run of test_train_py_end_to_end_on_the_emulated_kernels)


def test_train_py_saves_the_same_checkpoints_under_both_schedules_on_the_emulated_kernels(monkeypatch, tmp_path):
  """train.py with algorithm=RED and 12 pretraining iterations: PretrainPlan (the default) and `+pretraining.schedule=per_function` leave identical agent.pth and
  discriminator.pth."""
  b = _bodies(monkeypatch)
  calls = []
  real = b.il.PretrainPlan.run
  monkeypatch.setattr(b.il.PretrainPlan, 'run', lambda self, n: (calls.append(n), real(self, n))[1])
  out = b.train_both_schedules(tmp_path, ['algorithm=RED', 'env=hopper', 'imitation.pretraining.iterations=12'], SHORT, calls)
  assert calls == [12] and 'discriminator' in out


def test_epoch_binding_matches_the_compiled_library():
  """il_struct_size(12) is sizeof(il_epoch) as compiled; the ctypes mirror must agree, and the workspace of the general-shape entry point holds the per-function
  workspace plus the staging slab (n rows of states | actions | weights)."""
  import ctypes as C
  L = _lib.lib()
  assert L.il_struct_size(12) == C.sizeof(_lib.Epoch) == 24
  for S, A, H, depth, n in ((11, 3, 50, 2, 24), (11, 3, 48, 3, 32), (300, 12, 128, 2, 100)):
    assert L.il_bc_epoch_workspace_floats_general(S, A, H, depth, n) >= L.il_actor_workspace_floats_general(S, A, H, depth, n) + n * (S + A + 1)
