"""`-m gpu`: lockstep evaluation for general actor shapes - the launch `il_act_eval_rows_general` (csrc/general.hip k_act_eval_rows_general: gt_fwd_tile on every 16-row
tile), `il.GeneralLockstepEvaluator`, `evaluate_agent_lockstep` with a general actor and `+evaluation.schedule=lockstep` of train.py at a general actor shape. The oracle is
the existing per-function path, bit for bit: `il_actor_act_general(greedy=1)` on the same rows, `SoftActor.get_greedy_action` row by row and `evaluate_agent` on fresh
copies of the environments. Every comparison is exact. The bodies also run on the host emulation of the kernels (tests/test_lockstep_eval_general_emulated.py), whose
bounds checks cover the LDS sizing (gt_fwd_lds of the widest learner) and the mailbox layout. Bodies modelled on tests/test_lockstep_eval_gpu.py, whose layout helpers
and run watcher are used as they are."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_lockstep_eval_gpu as tle
from test_lockstep_eval_gpu import SENTINEL, _fill_sentinel, _layout, _views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib
  from gpu_util import DEV, N, Cfg

ACT = {'relu': 0, 'tanh': 1, 'sigmoid': 2}
# (S, A, H, depth, activation): the narrowest hidden (part ends where Os begins; no hidden-to-hidden layer) | hidden no multiple of 64, an odd number of cur / nxt swaps |
# general only by its width | an even number of swaps | the widest environment at the widest fused hidden, one layer deeper
SHAPES = [(11, 3, 16, 1, 'tanh'), (17, 6, 48, 3, 'tanh'), (27, 8, 96, 2, 'relu'), (18, 6, 64, 4, 'sigmoid'), (112, 8, 256, 3, 'relu')]
SHAPE_IDS = ['S11-A3-H16-d1-tanh', 'S17-A6-H48-d3-tanh', 'S27-A8-H96-d2-relu', 'S18-A6-H64-d4-sigmoid', 'S112-A8-H256-d3-relu']
WIDTHS = [(11, 3), (17, 6), (27, 8)]   # test 3: three learners at hidden 48, depth 3, tanh


def _actor(S, A, H, depth, activation, seed):
  torch.manual_seed(seed)
  actor = il.SoftActor(S, A, Cfg(hidden_size=H, depth=depth, activation=activation), device=DEV)
  assert actor.general
  actor.flat.copy_(torch.randn_like(actor.flat) * 0.08)
  return actor


def _fused_actor(S, A, H, seed):
  actor = il.SoftActor(S, A, Cfg(hidden_size=H, depth=2, activation='relu'), device=DEV)
  assert not actor.general
  return actor


def _reference_actions(actor, obs):
  """il_actor_act_general(greedy = 1) on the rows of `obs`, in one call."""
  n = obs.shape[0]
  states, out = torch.from_numpy(obs).to(DEV), torch.empty(n, actor.action_size, device=DEV)
  ws = torch.zeros(int(_lib.lib().il_actor_workspace_floats_general(actor.state_size, actor.action_size, actor.hidden, actor.depth, n)), device=DEV)
  _lib.check(_lib.lib().il_actor_act_general(_lib.ptr(actor.flat), actor.state_size, actor.action_size, actor.hidden, actor.depth, ACT[actor.activation], _lib.ptr(states), states.stride(0), n, None,
                                             C.c_uint64(0), 0, 1, _lib.ptr(out), None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
  return torch.from_numpy(N(out))


# ------------------------------------------------------------------------------------------------ 1. rows
def rows_equal_the_per_function_greedy_action(shape, n, full):
  S, A, H, depth, activation = shape
  max_rows = n if full else 48
  actor = _actor(S, A, H, depth, activation, 5)
  obs = np.random.RandomState(n).standard_normal((n, S)).astype(np.float32)
  ev = il.GeneralLockstepEvaluator([actor], max_rows)
  _fill_sentinel(ev)
  calls = actor._act_calls
  acts = ev.act([obs])[0]
  torch.cuda.synchronize()
  assert actor._act_calls == calls + n
  assert acts.shape == (n, A) and torch.equal(acts, _reference_actions(actor, obs))
  for r in range(n):
    assert torch.equal(acts[r:r + 1], torch.from_numpy(N(actor.get_greedy_action(torch.from_numpy(obs[r:r + 1]))))), f'row {r}'
  box, act, echo = _views(ev, 0)
  assert np.array_equal(act[:n, :A], acts.numpy())
  assert (act[n:] == SENTINEL).all(), 'a row >= n of the action block was written'
  assert (act[:, A:] == SENTINEL).all(), 'the padding of an action row was written'
  assert box[0] == ev.word and box[1] == n and (echo == ev.word).all() and len(echo) == (max_rows + 15) // 16
  assert (ev.L, ev.widths, ev.max_rows, ev.tiles, ev.actors) == (1, [(S, A)], max_rows, (max_rows + 15) // 16, [actor]) and ev.floats == _layout(S, A, max_rows)[6]


@pytest.mark.parametrize('full', [True, False], ids=['max_rows=n', 'max_rows=48'])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 33])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_rows_equal_the_per_function_greedy_action(shape, n, full):
  rows_equal_the_per_function_greedy_action(shape, n, full)


# ------------------------------------------------------------------------------------------------ 2. LDS opt-in
def test_rows_of_the_widest_shape_take_the_lds_opt_in():
  """S = 512, A = 8, hidden 512: gt_fwd_lds is 133,888 bytes, so the launch takes il_ensure_lds's opt-in (every shape of test 1 stays below 64 KiB)."""
  S, A, H, n = 512, 8, 512, 17
  actor = _actor(S, A, H, 2, 'tanh', 6)
  obs = np.random.RandomState(1).standard_normal((n, S)).astype(np.float32)
  ev = il.GeneralLockstepEvaluator([actor], n)
  _fill_sentinel(ev)
  acts = ev.act([obs])[0]
  torch.cuda.synchronize()
  assert torch.equal(acts, _reference_actions(actor, obs))
  _, act, echo = _views(ev, 0)
  assert np.array_equal(act[:n, :A], acts.numpy()) and (echo == ev.word).all() and (act[:, A:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ 3. learners
@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_learners_of_different_widths_equal_their_single_learner_launches(order):
  widths, counts = (WIDTHS, (17, 0, 5)) if order == 'forward' else (WIDTHS[::-1], (5, 0, 17))
  actors = [_actor(S, A, 48, 3, 'tanh', 20 + S) for S, A in widths]
  rs = np.random.RandomState(3)
  obs = [rs.standard_normal((n, S)).astype(np.float32) for n, (S, A) in zip(counts, widths)]
  ev = il.GeneralLockstepEvaluator(actors, 32)
  _fill_sentinel(ev)
  acts = ev.act(obs)
  torch.cuda.synchronize()
  for l, (n, (S, A)) in enumerate(zip(counts, widths)):
    box, act, echo = _views(ev, l)
    assert (echo == ev.word).all() and box[1] == n
    assert acts[l].shape == (n, A)
    if n == 0:
      assert (act == SENTINEL).all(), 'a learner without rows got more than its echoes'
      continue
    single = il.GeneralLockstepEvaluator([actors[l]], 32)
    _fill_sentinel(single)
    assert torch.equal(acts[l], single.act([obs[l]])[0]) and torch.equal(acts[l], _reference_actions(actors[l], obs[l]))
    torch.cuda.synchronize()
    _, act1, echo1 = _views(single, 0)
    assert act.tobytes() == act1.tobytes() and (echo1 == single.word).all(), f'learner {l}: its mailbox differs from its own single-learner launch'
    assert (act[n:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ 4. replay
def test_replayed_launch_second_post_and_sequence_wrap():
  S, A = 17, 6
  actor = _actor(S, A, 48, 3, 'tanh', 9)
  rs = np.random.RandomState(4)
  obs1, obs2 = (rs.standard_normal((19, S)).astype(np.float32) for _ in range(2))
  ev = il.GeneralLockstepEvaluator([actor], 40)
  _fill_sentinel(ev)
  a1 = ev.act([obs1])[0]
  torch.cuda.synchronize()
  first, word1 = ev.host.copy(), float(ev.word)
  ev.launch()   # again, without a new post: the same actions, the same echoes
  torch.cuda.synchronize()
  assert ev.host.tobytes() == first.tobytes()
  a2 = ev.act([obs2])[0]
  torch.cuda.synchronize()
  _, _, echo = _views(ev, 0)
  assert float(ev.word) == word1 + 64 and (echo == ev.word).all()
  assert not torch.equal(a1, a2) and torch.equal(a2, _reference_actions(actor, obs2))
  ev._seq = (1 << 17) - 2
  words = []
  for _ in range(3):
    a = ev.act([obs1])[0]
    words.append(float(ev.word))
    assert torch.equal(a, a1)
  torch.cuda.synchronize()
  assert words == [((1 << 17) - 1) * 64 + 4.0, 1 * 64 + 4.0, 2 * 64 + 4.0]   # 2^17 - 1 -> 1: never 0
  # a post that is never launched is not waited for: the next post replaces it at once, and the launch after it serves the later one
  ev.wait()
  ev.post([obs1])
  ev.post([obs2])
  assert not ev._in_flight and float(ev.word) == 4 * 64 + 4.0
  ev.launch()
  ev.wait()
  _, act, echo = _views(ev, 0)
  assert (echo == ev.word).all() and np.array_equal(act[:19, :A], a2.numpy())


# ------------------------------------------------------------------------------------------------ 5. refusals
_TILES_OFF = '''
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
class D(C.Structure): _fields_ = [('actor', C.c_void_p), ('mailbox', C.c_void_p), ('state_dim', C.c_int32), ('action_dim', C.c_int32)]
d = (D * 1)(D(4096, 8192, 18, 6))   # never dereferenced: the refusal is decided on the host records, before any launch
lib.il_act_eval_rows_general.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
lib.il_last_error.restype = C.c_char_p
rc = lib.il_act_eval_rows_general(C.cast(d, C.c_void_p), C.cast(d, C.c_void_p), 1, 16, 48, 3, 1, None)
print(rc, lib.il_last_error().decode())
'''


def _library_path():
  return _lib.LIB_PATH


def test_refusals_come_before_any_launch():
  from imitation_learning_amd.training import _device_array
  L = _lib.lib()
  S, A, H, depth, max_rows = 18, 6, 48, 3, 16
  actor = _actor(S, A, H, depth, 'tanh', 2)
  n = int(L.il_eval_mailbox_floats(S, A, max_rows))
  assert n == _layout(S, A, max_rows)[6]
  box = torch.zeros(n, dtype=torch.float32, pin_memory=True)
  box[:] = SENTINEL
  untouched = box.clone()

  def call(S=S, A=A, H=H, depth=depth, activation=1, max_rows=max_rows, actor_ptr=actor.flat.data_ptr(), box_ptr=box.data_ptr(), dev='ok', host='ok', L_=1, shift=0):
    d = _lib.EvalLearner(actor_ptr, box_ptr, S, A)
    host_arr = (_lib.EvalLearner * 1)(d)
    dev_arr = _device_array([d, d], DEV)   # (twice the record: room to hand over a misaligned address inside the allocation)
    p_dev = None if dev is None else C.c_void_p(dev_arr.data_ptr() + shift)
    p_host = None if host is None else C.cast(host_arr, C.c_void_p)
    rc = L.il_act_eval_rows_general(p_dev, p_host, L_, max_rows, H, depth, activation, torch.cuda.current_stream().cuda_stream)
    return rc, L.il_last_error().decode()

  ARG, UNSUPPORTED = 1, 2   # IL_ERR_ARG, IL_ERR_UNSUPPORTED (include/il_hip.h)
  for kw, code, words in ((dict(max_rows=0), ARG, 'max_rows=0'), (dict(max_rows=1025), ARG, 'max_rows=1025'), (dict(dev=None), ARG, 'null array'), (dict(host=None), ARG, 'null array'),
                          (dict(shift=4), ARG, 'not 8-byte aligned'), (dict(actor_ptr=None), ARG, 'learner 0: null pointer'), (dict(box_ptr=None), ARG, 'learner 0: null pointer'),
                          (dict(S=0), ARG, 'state_dim=0'), (dict(A=0), ARG, 'action_dim=0'), (dict(L_=0), ARG, 'n_learners=0'), (dict(L_=65536), ARG, 'n_learners=65536'),
                          (dict(depth=0), ARG, 'depth=0'), (dict(depth=9), ARG, 'depth=9'), (dict(activation=3), ARG, 'activation=3'), (dict(H=0), ARG, 'hidden=0'),
                          (dict(H=40), UNSUPPORTED, 'learner 0'), (dict(H=40), UNSUPPORTED, 'hidden=40'), (dict(H=528), UNSUPPORTED, 'hidden=528'),
                          (dict(S=513), UNSUPPORTED, 'state_dim=513'), (dict(A=9), UNSUPPORTED, 'action_dim=9'), (dict(A=9), UNSUPPORTED, 'no layer-at-a-time form')):
    rc, msg = call(**kw)
    assert rc == code and words in msg and 'il_act_eval_rows_general' in msg, (kw, rc, msg)
  # IL_GENERAL_TILES is read once per process: a process of its own, which needs no device (no refusal touches one)
  out = subprocess.run([sys.executable, '-c', _TILES_OFF, _library_path()], env=dict(os.environ, IL_GENERAL_TILES='0'), capture_output=True, text=True, timeout=120)
  assert out.returncode == 0 and out.stdout.startswith(f'{UNSUPPORTED} ') and 'IL_GENERAL_TILES' in out.stdout and 'learner 0' in out.stdout, (out.stdout, out.stderr)
  torch.cuda.synchronize()
  assert torch.equal(box, untouched), 'a refused call launched'
  box[0], box[1] = 68.0, 0.0   # and the same arguments, unedited, are served: a post without rows gets its echo and nothing else
  rc, msg = call()
  torch.cuda.synchronize()
  o_echo = _layout(S, A, max_rows)[2]
  assert rc == 0 and box[o_echo].item() == 68.0
  untouched[0], untouched[1], untouched[o_echo] = 68.0, 0.0, 68.0
  assert torch.equal(box, untouched)

  fused = _fused_actor(S, A, 64, 3)
  with pytest.raises(NotImplementedError, match='GeneralLockstepEvaluator: learner 0: not a general-shape actor'):
    il.GeneralLockstepEvaluator([fused], 4)
  with pytest.raises(NotImplementedError, match='GeneralLockstepEvaluator: learner 1: not a general-shape actor'):
    il.GeneralLockstepEvaluator([actor, fused], 4)
  with pytest.raises(NotImplementedError, match=r'one \(hidden, depth, activation\) for all learners'):
    il.GeneralLockstepEvaluator([actor, _actor(S, A, H, 4, 'tanh', 3)], 4)
  with pytest.raises(NotImplementedError, match='GeneralLockstepEvaluator: learner 0: hidden 40 is not a multiple of 16'):
    il.GeneralLockstepEvaluator([_actor(S, A, 40, depth, 'tanh', 3)], 4)
  for bad in (0, 1025):
    with pytest.raises(NotImplementedError, match=f'max_rows {bad} is outside 1..1024'):
      il.GeneralLockstepEvaluator([actor], bad)
  with pytest.raises(AssertionError, match='the mailbox holds 4'):
    il.GeneralLockstepEvaluator([actor], 4).act([np.zeros((5, S), np.float32)])
  with pytest.raises(NotImplementedError, match='LockstepEvaluator: learner 0: .*depth 2 / ReLU / hidden 64..256'):   # the fused evaluator's refusal of a general actor is what it was
    il.LockstepEvaluator([actor], 4)
  with pytest.raises(NotImplementedError, match='depth 2 / ReLU / hidden 64..256'):
    il.LockstepEvaluator([fused, actor], 4)


# ------------------------------------------------------------------------------------------------ 6. episodes
def test_episodes_of_different_lengths_equal_evaluate_agent_per_environment():
  from imitation_learning_amd.evaluation import evaluate_agent
  horizons, seeds = (5, 9, 7), (3, 3 + 7919, 3 + 2 * 7919)
  actor = _actor(18, 6, 48, 3, 'tanh', 31)
  calls = actor._act_calls
  returns, trajectories = il.evaluate_agent_lockstep(actor, tle._envs(horizons, seeds), 3, return_trajectories=True)   # evaluator=None: the general evaluator is built here
  torch.cuda.synchronize()
  assert actor._act_calls == calls + 21
  assert len(returns) == len(trajectories) == 3
  for k, env in enumerate(tle._envs(horizons, seeds)):
    ret, traj = evaluate_agent(actor, env, 1, True)
    assert returns[k] == ret[0], f'episode {k}'
    assert set(trajectories[k]) == set(traj[0])
    for key in traj[0]:
      assert torch.equal(trajectories[k][key], traj[0][key]), f'episode {k}: {key}'
    assert trajectories[k]['states'].shape == (horizons[k], 18)
  ev = il.GeneralLockstepEvaluator([actor], 3)
  assert il.evaluate_agent_lockstep(actor, tle._envs(horizons, seeds), 3, evaluator=ev) == returns   # the return shape without trajectories; an evaluator handed in


# ------------------------------------------------------------------------------------------------ 7. end to end
GENERAL = ['reinforcement.actor.depth=3', 'reinforcement.actor.activation=tanh', 'reinforcement.actor.hidden_size=48']


def train_schedules_leave_the_same_agent(tmp_path, short, episodes=2, horizon=60):
  """`train.py algorithm=SAC env=halfcheetah seed=3` with a depth-3 tanh hidden-48 actor, shortened, save_trajectories=true: the same agent.pth bytes under `sequential`
  and under `lockstep`; the lockstep run evaluated through evaluate_agent_lockstep (twice, and once more for the trajectories) and printed no `[train] evaluation:` line."""
  argv = ['algorithm=SAC', 'env=halfcheetah', 'seed=3'] + list(short) + GENERAL + [f'evaluation.episodes={episodes}', 'save_trajectories=true']
  seq, did_seq = tle._train(tmp_path, 'sequential', argv)
  lock, did_lock = tle._train(tmp_path, 'lockstep', argv + ['+evaluation.schedule=lockstep'])
  assert did_seq.counts() == {'evaluate_agent': 3}
  did_lock.assert_lockstep_served({'evaluate_agent_lockstep': 3})
  assert did_lock.calls['evaluate_agent_lockstep'] == [False, False, True]
  assert open(seq / 'agent.pth', 'rb').read() == open(lock / 'agent.pth', 'rb').read()
  ms, ml = (torch.load(d / 'metrics.pth', weights_only=False) for d in (seq, lock))
  assert ms['test_steps'] == ml['test_steps'] and len(ml['test_steps']) == 2
  assert all(len(r) == episodes for r in ml['test_returns'])
  assert ml['test_returns'][0][0] == ms['test_returns'][0][0]   # copy 0 is the sequential schedule's eval_env: the first episode it ever runs is the same episode
  for d in (seq, lock):
    tle._assert_trajectories(torch.load(d / 'trajectories.pth', weights_only=False), episodes, 18, 6, horizon)


def test_train_with_a_general_actor_under_both_evaluation_schedules(tmp_path):
  import test_train_gpu
  train_schedules_leave_the_same_agent(tmp_path, test_train_gpu.COMMON)
