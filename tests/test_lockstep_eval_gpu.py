"""`-m gpu`: lockstep evaluation - the launch `il_act_eval_rows` (csrc/sac.hip k_act_eval_rows), its mailbox (csrc/act_mail.hpp EvalMail), `il.LockstepEvaluator`,
`evaluate_agent_lockstep` / `evaluate_population_lockstep` and `+evaluation.schedule=lockstep` of train.py. The oracle is the existing per-function path, bit for bit:
`il_actor_act(greedy=1)` on the same rows, `SoftActor.get_greedy_action` row by row and `evaluate_agent` on fresh copies of the environments. Every comparison is exact.
The bodies also run on the host emulation of the kernels (tests/test_lockstep_eval_emulated.py), whose bounds checks cover the LDS sizing and the mailbox layout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib
  from gpu_util import DEV, N, Cfg

SENTINEL = -7.5   # no tanh value
SHAPES = [(11, 3, 64), (18, 6, 128), (112, 8, 256)]
WIDTHS = [(11, 3), (17, 6), (27, 8)]   # test 2 / 5: three learners at hidden 64


def _actor(S, A, H, seed):
  torch.manual_seed(seed)
  actor = il.SoftActor(S, A, Cfg(hidden_size=H, depth=2, activation='relu'), device=DEV)
  actor.flat.copy_(torch.randn_like(actor.flat) * 0.08)
  return actor


def _layout(S, A, max_rows):
  """The mailbox layout as include/il_hip.h states it, restated here: (obs offset, action offset, echo offset, Sp, Ap, tiles, floats)."""
  Sp, Ap, tiles = (S + 3) & ~3, (A + 3) & ~3, (max_rows + 15) // 16
  o_obs, o_act = 8, 8 + max_rows * Sp
  o_echo = o_act + max_rows * Ap
  return o_obs, o_act, o_echo, Sp, Ap, tiles, (o_echo + tiles + 15) & ~15


def _views(ev, l):
  """Learner l's mailbox of a LockstepEvaluator through the layout above (not through the evaluator's own views): (mailbox, action block [max_rows, Ap], echoes [tiles])."""
  S, A = ev.widths[l]
  o_obs, o_act, o_echo, Sp, Ap, tiles, floats = _layout(S, A, ev.max_rows)
  assert int(_lib.lib().il_eval_mailbox_floats(S, A, ev.max_rows)) == floats <= ev.floats
  box = ev.host[l]
  return box, box[o_act:o_echo].reshape(ev.max_rows, Ap), box[o_echo:o_echo + tiles]


def _fill_sentinel(ev):
  for l in range(ev.L):
    _, act, _ = _views(ev, l)
    act[:] = SENTINEL


def _reference_actions(actor, obs):
  """il_actor_act(greedy = 1) on the rows of `obs`, in one call."""
  n = obs.shape[0]
  states, out = torch.from_numpy(obs).to(DEV), torch.empty(n, actor.action_size, device=DEV)
  _lib.check(_lib.lib().il_actor_act(_lib.ptr(actor.flat), actor.state_size, actor.action_size, actor.hidden, _lib.ptr(states), states.stride(0), n, None, C.c_uint64(0), 0, 1, _lib.ptr(out), None,
                                     _lib.stream_ptr()))
  return torch.from_numpy(N(out))


# ------------------------------------------------------------------------------------------------ 1. rows
@pytest.mark.parametrize('full', [True, False], ids=['max_rows=n', 'max_rows=48'])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 33])
@pytest.mark.parametrize('shape', SHAPES, ids=['S11-A3-H64', 'S18-A6-H128', 'S112-A8-H256'])
def test_rows_equal_the_per_function_greedy_action(shape, n, full):
  S, A, H = shape
  max_rows = n if full else 48
  actor = _actor(S, A, H, 5)
  obs = np.random.RandomState(n).standard_normal((n, S)).astype(np.float32)
  ev = il.LockstepEvaluator([actor], max_rows)
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


def test_rows_of_a_state_wide_enough_for_the_lds_opt_in():
  """S = 700 at hidden 256: the tile's LDS passes 64 KiB, so the launch takes il_ensure_lds's opt-in (the other cases stay below it)."""
  S, A, H, n = 700, 4, 256, 17
  actor = _actor(S, A, H, 6)
  obs = np.random.RandomState(1).standard_normal((n, S)).astype(np.float32)
  ev = il.LockstepEvaluator([actor], n)
  _fill_sentinel(ev)
  acts = ev.act([obs])[0]
  torch.cuda.synchronize()
  assert torch.equal(acts, _reference_actions(actor, obs))
  _, act, echo = _views(ev, 0)
  assert (act[:, A:] == SENTINEL).all() and (echo == ev.word).all()


# ------------------------------------------------------------------------------------------------ 2. learners
@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_learners_of_different_widths_equal_their_single_learner_launches(order):
  widths, counts = (WIDTHS, (17, 0, 5)) if order == 'forward' else (WIDTHS[::-1], (5, 0, 17))
  actors = [_actor(S, A, 64, 20 + S) for S, A in widths]
  rs = np.random.RandomState(3)
  obs = [rs.standard_normal((n, S)).astype(np.float32) for n, (S, A) in zip(counts, widths)]
  ev = il.LockstepEvaluator(actors, 32)
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
    single = il.LockstepEvaluator([actors[l]], 32)
    assert torch.equal(acts[l], single.act([obs[l]])[0]) and torch.equal(acts[l], _reference_actions(actors[l], obs[l]))
    assert (act[n:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ 3. replay
def test_replayed_launch_second_post_and_sequence_wrap():
  S, A, H = 18, 6, 64
  actor = _actor(S, A, H, 9)
  rs = np.random.RandomState(4)
  obs1, obs2 = (rs.standard_normal((19, S)).astype(np.float32) for _ in range(2))
  ev = il.LockstepEvaluator([actor], 40)
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


# ------------------------------------------------------------------------------------------------ 4. episodes
def _envs(horizons, seeds, name='halfcheetah'):   # (halfcheetah: no early termination, so an episode's length is its horizon)
  from imitation_learning_amd.environments import SyntheticD4RLEnv
  envs = []
  for h, s in zip(horizons, seeds):
    env = SyntheticD4RLEnv(name, True, max_episode_steps=h)
    env.seed(s)
    envs.append(env)
  return envs


def test_episodes_of_different_lengths_equal_evaluate_agent_per_environment():
  from imitation_learning_amd.evaluation import evaluate_agent
  horizons, seeds = (5, 9, 7), (3, 3 + 7919, 3 + 2 * 7919)
  actor = _actor(18, 6, 64, 31)
  calls = actor._act_calls
  returns, trajectories = il.evaluate_agent_lockstep(actor, _envs(horizons, seeds), 3, return_trajectories=True)
  torch.cuda.synchronize()
  assert actor._act_calls == calls + 21
  assert len(returns) == len(trajectories) == 3
  for k, env in enumerate(_envs(horizons, seeds)):
    ret, traj = evaluate_agent(actor, env, 1, True)
    assert returns[k] == ret[0], f'episode {k}'
    assert set(trajectories[k]) == set(traj[0])
    for key in traj[0]:
      assert torch.equal(trajectories[k][key], traj[0][key]), f'episode {k}: {key}'
    assert trajectories[k]['states'].shape == (horizons[k], 18)
  assert il.evaluate_agent_lockstep(actor, _envs(horizons, seeds), 3) == returns   # the return shape without trajectories: a list of floats, episode order


# ------------------------------------------------------------------------------------------------ 5. population
def test_population_equals_evaluate_agent_lockstep_per_learner():
  names = ('hopper', 'halfcheetah', 'ant')   # absorbing bit on: S = 12, 18, 112 ... the population's widths are its environments'
  from imitation_learning_amd.environments import env_dims
  dims = [env_dims(n, True) for n in names]
  actors = [_actor(S, A, 64, 40 + S) for S, A in dims]
  horizons, make = (6, 11), lambda l: _envs((6, 11), (l, l + 7919), names[l])
  ev = il.LockstepEvaluator(actors, 2)
  calls = [a._act_calls for a in actors]
  got = il.evaluate_population_lockstep(ev, [make(l) for l in range(3)], 2)
  torch.cuda.synchronize()
  steps = [a._act_calls - c for a, c in zip(actors, calls)]
  for l in range(3):
    want = il.evaluate_agent_lockstep(actors[l], make(l), 2)
    assert got[l] == want and len(want) == 2, f'learner {l}'
  assert steps[1] == sum(horizons) and all(2 <= s <= sum(horizons) for s in steps)   # (halfcheetah never ends early)
  assert il.evaluate_population_lockstep(ev, [make(l) for l in range(3)], 0) == [[], [], []]


def test_population_of_the_three_widths():
  """Test 2's three learners (widths the environments do not have) through evaluate_population_lockstep: environments stubbed to those widths."""

  class Env:
    def __init__(self, S, horizon, seed):
      self.S, self.max_episode_steps, self.rs, self.t = S, horizon, np.random.RandomState(seed), 0
    def reset(self):
      self.t = 0
      return torch.from_numpy(self.rs.standard_normal((1, self.S)).astype(np.float32))
    def step(self, action):
      self.t += 1
      a = action.to('cpu', torch.float32).numpy()
      return torch.from_numpy((self.rs.standard_normal((1, self.S)) * 0.5 + a.sum()).astype(np.float32)), float(a.sum()), self.t >= self.max_episode_steps

  actors = [_actor(S, A, 64, 20 + S) for S, A in WIDTHS]
  make = lambda l: [Env(WIDTHS[l][0], 4 + l, 10 * l), Env(WIDTHS[l][0], 7 - l, 10 * l + 1)]
  ev = il.LockstepEvaluator(actors, 2)
  got = il.evaluate_population_lockstep(ev, [make(l) for l in range(3)], 2)
  for l in range(3):
    assert got[l] == il.evaluate_agent_lockstep(actors[l], make(l), 2), f'learner {l}'


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_come_before_any_launch():
  from imitation_learning_amd.training import _device_array
  L = _lib.lib()
  S, A, H, max_rows = 18, 6, 64, 16
  actor = _actor(S, A, H, 2)
  n = int(L.il_eval_mailbox_floats(S, A, max_rows))
  assert n == _layout(S, A, max_rows)[6]
  box = torch.zeros(n, dtype=torch.float32, pin_memory=True)
  box[:] = SENTINEL
  untouched = box.clone()

  def call(S=S, A=A, H=H, max_rows=max_rows, actor_ptr=actor.flat.data_ptr(), box_ptr=box.data_ptr(), dev='ok', host='ok', L_=1, shift=0):
    d = _lib.EvalLearner(actor_ptr, box_ptr, S, A)
    host_arr = (_lib.EvalLearner * 1)(d)
    dev_arr = _device_array([d, d], DEV)   # (twice the record: room to hand over a misaligned address inside the allocation)
    p_dev = None if dev is None else C.c_void_p(dev_arr.data_ptr() + shift)
    p_host = None if host is None else C.cast(host_arr, C.c_void_p)
    rc = L.il_act_eval_rows(p_dev, p_host, L_, max_rows, H, torch.cuda.current_stream().cuda_stream)
    return rc, L.il_last_error().decode()

  ARG = 1   # IL_ERR_ARG (include/il_hip.h)
  for kw, code, words in ((dict(H=96), ARG, 'hidden=96'), (dict(A=9), ARG, 'learner 0'), (dict(max_rows=0), ARG, 'max_rows=0'), (dict(max_rows=1025), ARG, 'max_rows=1025'),
                          (dict(dev=None), ARG, 'null array'), (dict(host=None), ARG, 'null array'), (dict(shift=4), ARG, 'not 8-byte aligned'),
                          (dict(actor_ptr=None), ARG, 'learner 0: null pointer'), (dict(box_ptr=None), ARG, 'learner 0: null pointer'), (dict(S=0), ARG, 'state_dim=0'),
                          (dict(L_=0), ARG, 'n_learners=0'), (dict(L_=65536), ARG, 'n_learners=65536'), (dict(S=300), ARG, 'state_dim 300')):
    rc, msg = call(**kw)
    assert rc == code and words in msg, (kw, rc, msg)
  torch.cuda.synchronize()
  assert torch.equal(box, untouched), 'a refused call launched'
  box[0], box[1] = 68.0, 0.0   # and the same arguments, unedited, are served: a post without rows gets its echo and nothing else
  rc, msg = call()
  torch.cuda.synchronize()
  o_echo = _layout(S, A, max_rows)[2]
  assert rc == 0 and box[o_echo].item() == 68.0
  untouched[0], untouched[1], untouched[o_echo] = 68.0, 0.0, 68.0
  assert torch.equal(box, untouched)

  general = il.SoftActor(S, A, Cfg(hidden_size=48, depth=3, activation='tanh'), device=DEV)
  with pytest.raises(NotImplementedError, match='depth 2 / ReLU / hidden 64..256'):
    il.LockstepEvaluator([actor, general], 4)
  for bad in (0, 1025):
    with pytest.raises(NotImplementedError, match=f'max_rows {bad} is outside 1..1024'):
      il.LockstepEvaluator([actor], bad)
  with pytest.raises(AssertionError, match='the mailbox holds 4'):
    il.LockstepEvaluator([actor], 4).act([np.zeros((5, S), np.float32)])


# ------------------------------------------------------------------------------------------------ 7. end to end
EVALUATORS = ('evaluate_agent', 'evaluate_population', 'evaluate_agent_lockstep', 'evaluate_population_lockstep')


class _Watch:
  """What a run did about evaluation: the calls of train.py's four evaluation functions (name -> [return_trajectories per call]) and what it wrote to stderr. The
  assertions below rest on these: a run that fell back to the sequential schedule, or never reached the lockstep functions, leaves the same files otherwise."""

  def __enter__(self):
    import contextlib, io
    if ROOT not in sys.path: sys.path.insert(0, ROOT)
    import train
    self.train, self.calls, self.saved, self.err = train, {n: [] for n in EVALUATORS}, {n: getattr(train, n) for n in EVALUATORS}, io.StringIO()
    for n in EVALUATORS:
      def spy(*a, _n=n, **k):
        self.calls[_n].append(bool(k.get('return_trajectories', a[3] if len(a) > 3 and _n.startswith('evaluate_agent') else False)))
        return self.saved[_n](*a, **k)
      setattr(train, n, spy)
    self.redirect = contextlib.redirect_stderr(self.err)
    self.redirect.__enter__()
    return self

  def __exit__(self, *exc):
    self.redirect.__exit__(*exc)
    for n in EVALUATORS: setattr(self.train, n, self.saved[n])
    sys.stderr.write(self.err.getvalue())

  def counts(self):
    return {n: len(c) for n, c in self.calls.items() if c}

  def assert_lockstep_served(self, expected):
    assert self.counts() == expected, (self.counts(), expected)
    assert '[train] evaluation:' not in self.err.getvalue(), self.err.getvalue()


def _train(tmp_path, name, argv):
  """One `python train.py ...` in this process from a fresh working directory and fresh process-wide update counters; returns the directory and what it did about evaluation."""
  if ROOT not in sys.path: sys.path.insert(0, ROOT)
  import train
  from imitation_learning_amd import config, training as il_training
  il_training._NOISE.clear(); il_training._WS.clear()
  d = tmp_path / name
  d.mkdir()
  before = os.getcwd()
  os.chdir(d)
  try:
    with _Watch() as watch:
      assert np.isfinite(train.train(config.compose(argv)))
  finally:
    os.chdir(before)
  return d, watch


def _assert_trajectories(trajectories, episodes, S, A, horizon=None):
  """evaluate_agent's trajectory format: one dict per episode, in episode order."""
  assert isinstance(trajectories, list) and len(trajectories) == episodes
  for t in trajectories:
    assert set(t) == {'states', 'actions', 'rewards', 'terminals'}
    n = t['rewards'].numel()
    assert 1 <= n and (horizon is None or n == horizon)
    assert t['states'].shape == (n, S) and t['actions'].shape == (n, A) and t['terminals'].shape == (n,)
    assert t['terminals'][-1] == 1 and t['terminals'][:-1].sum() == 0 and torch.isfinite(t['states']).all() and (t['actions'].abs() <= 1).all()


def train_schedules_leave_the_same_agent(tmp_path, short, episodes=2, horizon=60):
  argv = ['algorithm=SAC', 'env=halfcheetah', 'seed=3'] + list(short) + [f'evaluation.episodes={episodes}']
  seq, did_seq = _train(tmp_path, 'sequential', argv)
  lock, did_lock = _train(tmp_path, 'lockstep', argv + ['+evaluation.schedule=lockstep'])
  assert did_seq.counts() == {'evaluate_agent': 2}   # the sequential schedule is the code it always was ...
  did_lock.assert_lockstep_served({'evaluate_agent_lockstep': 2})   # ... and lockstep is served by the lockstep function, not by a fallback
  assert open(seq / 'agent.pth', 'rb').read() == open(lock / 'agent.pth', 'rb').read()
  ms, ml = (torch.load(d / 'metrics.pth', weights_only=False) for d in (seq, lock))
  assert ms['test_steps'] == ml['test_steps'] and len(ml['test_steps']) == 2
  assert all(len(r) == episodes for r in ml['test_returns']) and all(len(r) == episodes for r in ml['test_returns_normalized'])
  assert ml['test_returns'][0][0] == ms['test_returns'][0][0]   # copy 0 is the sequential schedule's eval_env: the first episode it ever runs is the same episode
  assert ml['test_returns'][0][1] != ms['test_returns'][0][1]   # episode 1 runs on copy 1 (its own seed), not on the continued stream of copy 0
  assert all(isinstance(r, float) and np.isfinite(r) for ev in ml['test_returns'] for r in ev)
  # the final save_trajectories pass goes through the lockstep function too
  traj, did_traj = _train(tmp_path, 'lockstep_trajectories', argv + ['+evaluation.schedule=lockstep', 'save_trajectories=true'])
  did_traj.assert_lockstep_served({'evaluate_agent_lockstep': 3})
  assert did_traj.calls['evaluate_agent_lockstep'] == [False, False, True]
  _assert_trajectories(torch.load(traj / 'trajectories.pth', weights_only=False), episodes, 18, 6, horizon)
  assert open(traj / 'agent.pth', 'rb').read() == open(lock / 'agent.pth', 'rb').read()
  return ms, ml


def test_train_under_both_evaluation_schedules(tmp_path):
  import test_train_gpu
  train_schedules_leave_the_same_agent(tmp_path, test_train_gpu.COMMON)


def sweep_schedules_leave_the_same_bytes_under_lockstep(tmp_path, short, tp, episodes=2, horizon=60):
  """`-m seed=3,4` with +evaluation.schedule=lockstep and save_trajectories=true: the population schedule evaluates through ONE evaluator (evaluate_population_lockstep) and
  saves each learner's trajectories through an evaluator of its own; per_learner evaluates learner by learner (evaluate_agent_lockstep). The same bytes."""
  argv = ['-m', 'seed=3,4', 'algorithm=SAC', 'env=halfcheetah'] + list(short) + [f'evaluation.episodes={episodes}', '+evaluation.schedule=lockstep', 'save_trajectories=true']
  with _Watch() as did_p:
    root_p, scores_p = tp._sweep(tmp_path, 'population', argv + ['+sweep.schedule=population'])
  with _Watch() as did_l:
    root_l, scores_l = tp._sweep(tmp_path, 'per_learner', argv + ['+sweep.schedule=per_learner'])
  did_p.assert_lockstep_served({'evaluate_population_lockstep': 2, 'evaluate_agent_lockstep': 2})
  did_l.assert_lockstep_served({'evaluate_agent_lockstep': 6})
  assert np.isfinite(scores_p).all() and scores_p == scores_l
  for j in (0, 1):
    fp, fl = tp._job_files(root_p, j), tp._job_files(root_l, j)
    assert set(fp) == set(fl) == {'agent.pth', 'metrics.pth', 'trajectories.pth'}
    for f in ('agent.pth', 'metrics.pth'):
      a, b = ({k: v for k, v in m.items() if k not in tp.TIMING_KEYS} for m in (fp[f], fl[f]))
      tp._assert_same_nested(a, b, f'job {j}: {f}')
    tp._assert_same_nested(fp['trajectories.pth'], fl['trajectories.pth'], f'job {j}: trajectories.pth')
    _assert_trajectories(fp['trajectories.pth'], episodes, 18, 6, horizon)
    assert all(len(r) == episodes for r in fp['metrics.pth']['test_returns']) and len(fp['metrics.pth']['test_steps']) == 2


def test_sweep_under_lockstep_evaluation_leaves_the_same_bytes_under_both_sweep_schedules(tmp_path):
  import test_population_acting_gpu as tp
  import test_train_gpu
  sweep_schedules_leave_the_same_bytes_under_lockstep(tmp_path, test_train_gpu.COMMON, tp)


def train_all_schedules_leave_the_same_bytes_under_lockstep(tmp_path, short, tmx, episodes=2):
  """`train_all.py algorithm=SAC seed=3` with +evaluation.schedule=lockstep: four learners of different widths through ONE evaluator under the population schedule, one
  evaluator each under per_learner; the same bytes, trajectories of each environment's own widths."""
  from imitation_learning_amd.environments import env_dims
  argv = ['algorithm=SAC', 'seed=3'] + list(short) + [f'evaluation.episodes={episodes}', '+evaluation.schedule=lockstep', 'save_trajectories=true']
  with _Watch() as did_p:
    root_p, scores_p, _ = tmx._train_all(tmp_path, 'population', argv + ['+sweep.schedule=population'])
  with _Watch() as did_l:
    root_l, scores_l, _ = tmx._train_all(tmp_path, 'per_learner', argv + ['+sweep.schedule=per_learner'])
  did_p.assert_lockstep_served({'evaluate_population_lockstep': 2, 'evaluate_agent_lockstep': 4})
  did_l.assert_lockstep_served({'evaluate_agent_lockstep': 12})
  assert np.isfinite(list(scores_p.values())).all() and scores_p == scores_l
  fp, fl = tmx._env_files(root_p), tmx._env_files(root_l)
  tmx._assert_same_runs({e: {f: v for f, v in d.items() if f != 'trajectories.pth'} for e, d in fp.items()},
                        {e: {f: v for f, v in d.items() if f != 'trajectories.pth'} for e, d in fl.items()}, 'lockstep: population against per_learner', {'agent.pth', 'metrics.pth'})
  for env in tmx.ENVS:
    tmx.tp._assert_same_nested(fp[env]['trajectories.pth'], fl[env]['trajectories.pth'], f'{env}: trajectories.pth')
    _assert_trajectories(fp[env]['trajectories.pth'], episodes, *env_dims(env, True))
    assert all(len(r) == episodes for r in fp[env]['metrics.pth']['test_returns']) and len(fp[env]['metrics.pth']['test_steps']) == 2


def test_train_all_under_lockstep_evaluation(tmp_path):
  import test_mixed_population_gpu as tmx
  train_all_schedules_leave_the_same_bytes_under_lockstep(tmp_path, tmx.COMMON, tmx)
