"""`-m gpu` integration: train.py with a general-shape actor (reinforcement.actor.depth=3, activation=tanh) acts through the acting worker (il_act_step_general) instead of
dropping to the per-function path. The exact schedule is the reference order, so it must train the same learner as `+acting.schedule=per_function`, bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from test_train_gpu import COMMON   # noqa: E402  (the short step counts of tests/test_train_gpu.py)

GENERAL = ['algorithm=SAC', 'env=hopper', 'reinforcement.actor.depth=3', 'reinforcement.actor.activation=tanh']
TRACED_LAUNCHES = 6   # acting launches traced at the start of a run (before training.start: nothing is being captured yet)


def _train(tmp_path, name, extra, monkeypatch=None):
  """One train.py run in its own directory. With `monkeypatch`: the library's launch trace (il_trace_enable / il_trace_report) is on for the first acting launches of
  the run, and the kernel names it saw are returned - train.py itself and everything it writes are untouched."""
  sys.path.insert(0, ROOT)
  import train
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib, config
  seen = {}
  if monkeypatch is not None:
    launch, calls = il.ActingWorker._launch, [0]

    def traced(self, *a, **k):
      L = _lib.lib()
      if calls[0] == 0: L.il_trace_enable(1)
      launch(self, *a, **k)
      calls[0] += 1
      if calls[0] == TRACED_LAUNCHES:
        buf = C.create_string_buffer(1 << 14)
        _lib.check(L.il_trace_report(buf, len(buf)))
        L.il_trace_enable(0)
        for line in buf.value.decode().strip().splitlines():
          kernel, count, _ = line.split()
          seen[kernel] = int(count)
    monkeypatch.setattr(il.ActingWorker, '_launch', traced)
  from imitation_learning_amd import training as il_training
  il_training._NOISE.clear(); il_training._WS.clear()   # the update noise counter lives with the process: every run starts from zero, like a fresh `python train.py`
  d = tmp_path / name
  d.mkdir()
  os.chdir(d)
  score = train.train(config.compose(GENERAL + list(extra) + COMMON))
  if monkeypatch is not None: monkeypatch.undo()
  agent = torch.load(d / 'agent.pth', weights_only=False)
  metrics = torch.load(d / 'metrics.pth', weights_only=False)
  return score, agent, metrics, seen


def _same(a, b, what):
  assert set(a) == set(b), what
  for k in a:
    np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=f'{what}: {k}')


def test_default_schedule_trains_the_per_function_learner_through_the_one_launch_worker(tmp_path, monkeypatch):
  """The default schedule (exact: act -> env.step -> append -> update, the reference order) against +acting.schedule=per_function: the saved actor, critic and
  log_alpha bit-identical, and the default run's acting launches were k_act_step_general (the library's launch trace over its first launches)."""
  score_w, agent_w, metrics_w, seen = _train(tmp_path, 'worker', [], monkeypatch)
  assert seen.get('k_act_step_general') == TRACED_LAUNCHES and set(seen) == {'k_act_step_general'}, seen
  score_p, agent_p, metrics_p, _ = _train(tmp_path, 'per_function', ['+acting.schedule=per_function'])
  assert np.isfinite(score_w) and score_w == score_p
  for part in ('actor', 'critic'):
    _same(agent_w[part], agent_p[part], part)
  np.testing.assert_array_equal(np.asarray(agent_w['log_alpha'].cpu()), np.asarray(agent_p['log_alpha'].cpu()))
  assert len(metrics_w['update_steps']) >= 2 and metrics_w['train_returns'] == metrics_p['train_returns']


@pytest.mark.parametrize('schedule', ['fused', 'overlap'])
def test_fused_and_overlap_schedules_run_with_a_general_actor(tmp_path, schedule):
  score, agent, metrics, _ = _train(tmp_path, schedule, [f'+acting.schedule={schedule}'])
  assert np.isfinite(score)
  assert all(torch.isfinite(v).all() for v in agent['actor'].values()) and all(torch.isfinite(v).all() for v in agent['critic'].values())
  assert len(metrics['update_steps']) >= 2 and all(np.isfinite(q).all() for q in metrics['Q_values']) and all(np.isfinite(e).all() for e in metrics['entropies'])
