"""`-m gpu`: the population acting launch (`il_act_step_population`, csrc/sac.hip) and its worker (`il.PopulationActingWorker`): L learners of one fused actor shape, ONE
launch per lockstep environment step. The oracle is the existing per-learner path - one `il.ActingWorker(noise_seed=seed_l)` per learner - bit for bit: actions, whole
rings, device cursors, host mirrors and Philox counters. Then the seed sweep of train.py (`-m seed=...`) under both of its schedules, which must leave the same bytes.
The bodies of the kernel-level cases also run on the host emulation of the kernels (tests/test_population_acting_emulated.py), whose lanes do not run in lockstep."""
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

CAPACITY, STEPS = 37, 60


def _actors_and_memories(S, A, H, L, absorbing, capacity=CAPACITY):
  """Two identical sets of L actors (different parameters per learner) and L empty rings each."""
  cfg = Cfg(hidden_size=H, depth=2, activation='relu')
  sets = ([], [])
  for l in range(L):
    torch.manual_seed(11 + l)
    flat = None
    for side in sets:
      actor = il.SoftActor(S, A, cfg, device=DEV)
      if flat is None: flat = torch.randn_like(actor.flat) * 0.08
      actor.flat.copy_(flat)
      side.append(actor)
  mems = tuple([il.ReplayMemory(capacity, S, A, absorbing, device=DEV) for _ in range(L)] for _ in range(2))
  return sets[0], sets[1], mems[0], mems[1]


def _last_row_step(absorbing, first_end):
  """The step whose transition lands on row CAPACITY - 1 when one true termination (at `first_end`, one extra row with absorbing=true) precedes it."""
  return CAPACITY - 1 if absorbing and first_end < CAPACITY - 1 else CAPACITY


def _learner_script(l, n, S, absorbing, last_row=False):
  """test_gpu_parity._episode_script with learner l's own data and its episode ends shifted by l: (next_obs, reward, true_terminal, timeout) per step, the first
  observation and the reset observations. `last_row`: the second true termination is the transition written to the ring's last row."""
  rs = np.random.RandomState(100 + l)
  terms, touts = {7 + l, 31 + l, 52 + l}, {19 + l, 44 + l}
  if last_row:
    terms = {7 + l, _last_row_step(absorbing, 7 + l), 52 + l}
  script = []
  for t in range(1, n + 1):
    obs = rs.standard_normal(S).astype(np.float32)
    if absorbing: obs[-1] = 0.0
    script.append((obs, float(rs.standard_normal()), t in terms, t in touts))
  first = rs.standard_normal(S).astype(np.float32)
  resets = [rs.standard_normal(S).astype(np.float32) * 0.1 for _ in range(8)]
  if absorbing:
    first[-1] = 0.0
    for r in resets: r[-1] = 0.0
  return script, first, resets


def _rows_of_true_terminations(script, absorbing):
  """Ring row of every true termination of a script (the cursor arithmetic of memory.py:40-44, 65-68)."""
  cursor, rows = 0, []
  for (_, _, term, tout) in script:
    if term and not tout: rows.append(cursor % CAPACITY)
    cursor += 2 if (absorbing and term and not tout) else 1
  return rows


def _run_single(worker, schedule, script, first, resets):
  """One learner through its own ActingWorker: the loop of test_acting_worker_matches_separate_calls."""
  acts, k = [], 0
  if schedule == 'exact':
    obs = first
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts.append(N(worker.act(obs)))
      worker.append(t, nxt, rew, term, tout)
      if term or tout: obs = resets[k]; k += 1
      else: obs = nxt
  else:
    a = worker.act(first)
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts.append(N(a))
      ended = term or tout
      a = worker.step(t, nxt, rew, term, tout, obs=resets[k] if ended else None)
      k += int(ended)
  return np.concatenate(acts)


class _Lockstep:
  """L scripts driven through one PopulationActingWorker; a learner can be paused (it idles in the launch) and a launch can be issued twice."""

  def __init__(self, worker, schedule, scripts):
    self.w, self.schedule, self.scripts, self.L = worker, schedule, scripts, worker.L
    self.t = [0] * self.L                     # transitions done per learner
    self.k = [0] * self.L                     # resets used
    self.obs = [s[1] for s in scripts]        # the observation each learner acts on next
    self.acts = [[] for _ in range(self.L)]
    self.pending = None                       # fused: the actions of the last launch
    if schedule == 'fused':
      self.pending = worker.act(self.obs)

  def _transition(self, l):
    script, _, resets = self.scripts[l]
    nxt, rew, term, tout = script[self.t[l]]
    self.t[l] += 1
    follow = nxt
    if term or tout:
      follow = resets[self.k[l]]; self.k[l] += 1
    return nxt, rew, term, tout, follow

  def launch(self, active, repeat=False):
    """One lockstep environment step of the learners in `active` (the others idle)."""
    w, L = self.w, self.L
    none = [None] * L
    if self.schedule == 'exact':
      a = w.act([self.obs[l] if l in active else None for l in range(L)])
      if repeat: w._launch(w._act_box); torch.cuda.synchronize()
      nxt, rew, term, tout, steps = list(none), [0.0] * L, [False] * L, [False] * L, [0] * L
      for l in active:
        self.acts[l].append(N(a[l:l + 1]))
        nxt[l], rew[l], term[l], tout[l], self.obs[l] = self._transition(l)
        steps[l] = self.t[l]
      w.append(steps, nxt, rew, term, tout)
      if repeat: w._launch(w._append_box); torch.cuda.synchronize()
    else:
      nxt, rew, term, tout, steps, obs = list(none), [0.0] * L, [False] * L, [False] * L, [0] * L, list(none)
      for l in active:
        self.acts[l].append(N(self.pending[l:l + 1]))
        nxt[l], rew[l], term[l], tout[l], obs[l] = self._transition(l)
        steps[l] = self.t[l]
      a = w.step(steps, nxt, rew, term, tout, obs=obs)
      if repeat: w._launch(w._act_box); torch.cuda.synchronize()
      self.pending = self.pending.clone()
      for l in active: self.pending[l] = a[l]

  def actions(self, l):
    return np.concatenate(self.acts[l])


def _assert_learners_equal(acts_ref, acts_pop, actors_a, actors_b, mems_a, mems_b):
  for l, (ma, mb) in enumerate(zip(mems_a, mems_b)):
    np.testing.assert_array_equal(acts_ref[l], acts_pop[l], err_msg=f'actions of learner {l}')
    np.testing.assert_array_equal(N(ma.ring), N(mb.ring), err_msg=f'ring of learner {l}')
    np.testing.assert_array_equal(N(ma._ring_state), N(mb._ring_state), err_msg=f'device cursor of learner {l}')
    assert (ma.idx, ma.full, ma.num_trajectories) == (mb.idx, mb.full, mb.num_trajectories), l
    assert N(mb._ring_state).tolist() == [mb.idx, int(mb.full), mb.size], l
    assert actors_a[l]._act_calls == actors_b[l]._act_calls, l


POPULATION_SHAPES = [pytest.param((18, 6, 256, 3), id='S18-A6-H256-L3'), pytest.param((111, 8, 64, 9), id='S111-A8-H64-L9')]


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
@pytest.mark.parametrize('shape', POPULATION_SHAPES)
def test_population_acting_matches_per_learner_workers(shape, schedule, absorbing):
  """60 lockstep steps of L learners into rings of 37 rows: every learner has its own episode script (ends shifted by the learner index, so one launch mixes wrapping,
  plain and ending learners; learner 1's second true termination is written to the ring's last row, its absorbing row to row 0), its own actor parameters and Philox seed.
  (111, 8, 64, 9): a 235-float row spread over the four waves of the workgroup, and more learners than XCDs."""
  S, A, H, L = shape
  actors_a, actors_b, mems_a, mems_b = _actors_and_memories(S, A, H, L, absorbing)
  scripts = [_learner_script(l, STEPS, S, absorbing, last_row=l == 1) for l in range(L)]
  seeds = [1000 + 17 * l for l in range(L)]
  assert CAPACITY - 1 in _rows_of_true_terminations(scripts[1][0], absorbing), 'a true termination is meant to land on the last row of the ring'

  acts_ref = [_run_single(il.ActingWorker(actors_a[l], mems_a[l], noise_seed=seeds[l]), schedule, *scripts[l]) for l in range(L)]

  run = _Lockstep(il.PopulationActingWorker(actors_b, mems_b, seeds), schedule, scripts)
  for _ in range(STEPS):
    run.launch(list(range(L)))
  torch.cuda.synchronize()
  _assert_learners_equal(acts_ref, [run.actions(l) for l in range(L)], actors_a, actors_b, mems_a, mems_b)
  assert all(m.full for m in mems_b), 'the scripts are meant to wrap every ring'
  assert not np.array_equal(N(mems_b[0].ring), N(mems_b[1].ring)) and not np.array_equal(acts_ref[0], acts_ref[1]), 'the learners are meant to differ'


@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_population_acting_idle_learner_and_repeated_launches(schedule, shape=(18, 6, 64, 3)):
  """Learner 1 (a 40-step script; the others have 50 steps) idles for launches 15..24 - a post with neither PENDING nor an action - while the others act, with a
  transition of its own in flight under the fused schedule, and every launch of steps 5, 20 and 30 is issued twice without a new post: each learner's actions, ring,
  cursor and counters are those of its own ActingWorker running its script straight through, and nothing of the idle learner moves while it idles."""
  S, A, H, L = shape
  absorbing = True
  actors_a, actors_b, mems_a, mems_b = _actors_and_memories(S, A, H, L, absorbing)
  lengths = [50 if l != 1 else 40 for l in range(L)]
  scripts = [_learner_script(l, lengths[l], S, absorbing) for l in range(L)]
  seeds = [77 + l for l in range(L)]
  acts_ref = [_run_single(il.ActingWorker(actors_a[l], mems_a[l], noise_seed=seeds[l]), schedule, *scripts[l]) for l in range(L)]

  w = il.PopulationActingWorker(actors_b, mems_b, seeds)
  run = _Lockstep(w, schedule, scripts)
  untouched = None
  for launch in range(1, 51):
    active = [l for l in range(L) if not (l == 1 and 15 <= launch <= 24)]
    if launch == 15:
      torch.cuda.synchronize()
      untouched = (N(w.carry[1]).copy(), N(mems_b[1].ring).copy(), N(mems_b[1]._ring_state).copy(), actors_b[1]._act_calls)
    if launch == 25:
      torch.cuda.synchronize()
      assert np.array_equal(untouched[0], N(w.carry[1])) and np.array_equal(untouched[1], N(mems_b[1].ring)) and np.array_equal(untouched[2], N(mems_b[1]._ring_state))
      assert untouched[3] == actors_b[1]._act_calls, 'an idle learner draws no noise'
    run.launch(active, repeat=launch in (5, 20, 30))
  assert run.t == lengths
  torch.cuda.synchronize()
  _assert_learners_equal(acts_ref, [run.actions(l) for l in range(L)], actors_a, actors_b, mems_a, mems_b)
  assert all(m.full for m in mems_b)


def test_population_greedy_and_evaluate_population():
  """Three hopper-shaped synthetic environments with different horizons (20, 35, 50: different episode lengths and an idle tail): evaluate_population returns
  evaluate_agent's lists, leaves every `_act_calls` where evaluate_agent leaves it and does not touch the carries of the transitions in flight; a greedy `act` is
  get_greedy_action."""
  from imitation_learning_amd.environments import SyntheticD4RLEnv
  from imitation_learning_amd.evaluation import evaluate_agent, evaluate_population
  horizons, absorbing, episodes = (20, 35, 50), True, 2
  envs_a = [SyntheticD4RLEnv('hopper', absorbing, max_episode_steps=h) for h in horizons]
  envs_b = [SyntheticD4RLEnv('hopper', absorbing, max_episode_steps=h) for h in horizons]
  for l, (ea, eb) in enumerate(zip(envs_a, envs_b)):
    ea.seed(40 + l); eb.seed(40 + l)
  S, A, L = envs_a[0].observation_space.shape[0], envs_a[0].action_space.shape[0], len(horizons)
  actors_a, actors_b, mems_a, mems_b = _actors_and_memories(S, A, 64, L, absorbing)
  seeds = [5, 6, 7]
  rs = np.random.RandomState(9)
  first = [rs.standard_normal(S).astype(np.float32) for _ in range(L)]
  for f in first: f[-1] = 0.0

  singles = [il.ActingWorker(actors_a[l], mems_a[l], noise_seed=seeds[l]) for l in range(L)]
  sampled_a = [N(singles[l].act(first[l])) for l in range(L)]   # a transition in flight: its (state, action) sit in the carry
  want = [evaluate_agent(actors_a[l], envs_a[l], episodes) for l in range(L)]

  w = il.PopulationActingWorker(actors_b, mems_b, seeds)
  sampled_b = N(w.act(first))
  torch.cuda.synchronize()
  carry = N(w.carry).copy()
  got = evaluate_population(w, envs_b, episodes)
  torch.cuda.synchronize()
  assert got == want and all(len(g) == episodes for g in got)
  assert len({len(g) for g in got}) == 1 and [a._act_calls for a in actors_a] == [b._act_calls for b in actors_b]
  assert len({a._act_calls for a in actors_b}) > 1, 'the episodes are meant to differ in length between the learners'
  np.testing.assert_array_equal(carry, N(w.carry), err_msg='evaluation must not touch the training carries')
  np.testing.assert_array_equal(np.concatenate(sampled_a), sampled_b)
  for l in range(L):
    np.testing.assert_array_equal(N(singles[l].carry)[:S + A], N(w.carry[l])[:S + A])

  # the transition in flight is appended as if no evaluation had happened, and a greedy act is get_greedy_action
  nxt = [rs.standard_normal(S).astype(np.float32) for _ in range(L)]
  for l in range(L):
    singles[l].append(1, nxt[l], 0.5 + l, False, False)
  w.append(1, nxt, [0.5 + l for l in range(L)], [False] * L, [False] * L)
  greedy = N(w.act(nxt, greedy=True))
  torch.cuda.synchronize()
  for l in range(L):
    np.testing.assert_array_equal(N(mems_a[l].ring), N(mems_b[l].ring))
    np.testing.assert_array_equal(N(actors_a[l].get_greedy_action(torch.from_numpy(nxt[l]))), greedy[l:l + 1])


def test_population_acting_loud_failures():
  L = _lib.lib()
  some = torch.zeros(64, dtype=torch.float32, device=DEV)
  for args, word in (((None, 3, 18, 6, 256, None), b'null'), ((_lib.ptr(some), 0, 18, 6, 256, None), b'no learner'), ((_lib.ptr(some), 3, 18, 6, 96, None), b'unsupported dims'),
                     ((_lib.ptr(some), 3, 18, 6, 320, None), b'unsupported dims'), ((_lib.ptr(some), 3, 300, 4, 64, None), b'exceed')):
    assert L.il_act_step_population(*args) != 0
    assert b'il_act_step_population' in L.il_last_error() and word in L.il_last_error(), L.il_last_error()
  actors, _, mems, _ = _actors_and_memories(18, 6, 64, 2, True)

  class Reward:   # stands for a PWILDiscriminator: the population launch has no coupling launch in front of it
    pass
  with pytest.raises(NotImplementedError, match='PWIL'):
    il.PopulationActingWorker(actors, mems, [1, 2], reward_models=[Reward(), Reward()])
  general = il.SoftActor(18, 6, Cfg(hidden_size=48, depth=3, activation='tanh'), device=DEV)
  with pytest.raises(NotImplementedError, match='population launch'):
    il.PopulationActingWorker([general, general], mems, [1, 2])


def test_act_learner_descriptor_abi():
  assert C.sizeof(_lib.ActLearner) == 5 * 8 + 8
  assert _lib.lib().il_struct_size(13) == C.sizeof(_lib.ActLearner)


# ---------------------------------------------------------------------------------------------
# train.py -m seed=...: the sweep as one population, population schedule against per_learner
# ---------------------------------------------------------------------------------------------
from test_train_gpu import COMMON  # noqa: E402  (steps 260, batch 64, two evaluations of two episodes, 60-step episodes)

TIMING_KEYS = ('training_time', 'pre_training_time')


def _sweep(tmp_path, name, argv):
  """One `python train.py -m ...` in this process, from a fresh working directory and fresh process-wide update counters; returns the sweep directory and the scores."""
  if ROOT not in sys.path: sys.path.insert(0, ROOT)
  import train
  from imitation_learning_amd import training as il_training
  il_training._NOISE.clear(); il_training._WS.clear()   # the update noise counters live with the process: every run starts from zero, like a fresh `python train.py`
  d = tmp_path / name
  d.mkdir()
  before = os.getcwd()
  os.chdir(d)
  try:
    return train.multirun(argv, stamp=name)
  finally:
    os.chdir(before)   # the tests after this one run from where they would have run


def _assert_same_nested(a, b, what):
  if isinstance(a, dict):
    assert set(a) == set(b), what
    for k in a: _assert_same_nested(a[k], b[k], f'{what}.{k}')
  elif isinstance(a, (list, tuple)):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)): _assert_same_nested(x, y, f'{what}[{i}]')
  elif torch.is_tensor(a):
    assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), what
  elif isinstance(a, np.ndarray):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
  else:
    assert a == b or (a != a and b != b), what


def _job_files(root, j):
  return {f: torch.load(os.path.join(root, str(j), f), weights_only=False) for f in sorted(os.listdir(os.path.join(root, str(j)))) if f.endswith('.pth')}


def sweep_schedules_leave_the_same_bytes(tmp_path, args, seeds, extra):
  """`-m seed=...` under +sweep.schedule=population and under per_learner: every job directory holds the same bytes of every tensor of agent.pth / discriminator.pth and the
  same metrics.pth entries (timing keys aside); the jobs differ from each other; the scores are finite."""
  argv = ['-m', 'seed=' + ','.join(str(s) for s in seeds)] + args + extra
  root_p, scores_p = _sweep(tmp_path, 'population', argv + ['+sweep.schedule=population'])
  root_l, scores_l = _sweep(tmp_path, 'per_learner', argv + ['+sweep.schedule=per_learner'])
  assert os.path.basename(os.path.dirname(root_p)) == f'{args[0].split("=")[1]}_{args[1].split("=")[1]}_sweeper'
  assert sorted(os.listdir(root_p)) == [str(j) for j in range(len(seeds))] == sorted(os.listdir(root_l))
  assert np.isfinite(scores_p).all() and scores_p == scores_l
  jobs = []
  for j in range(len(seeds)):
    fp, fl = _job_files(root_p, j), _job_files(root_l, j)
    assert set(fp) == set(fl) == {'agent.pth', 'metrics.pth'} | ({'discriminator.pth'} if 'algorithm=GAIL' in args else set())
    for f in fp:
      a, b = fp[f], fl[f]
      if f == 'metrics.pth':
        a, b = ({k: v for k, v in m.items() if k not in TIMING_KEYS} for m in (a, b))
        assert len(a['update_steps']) >= 2 and len(a['test_steps']) == 2 and all(np.isfinite(q).all() for q in a['Q_values'])
      _assert_same_nested(a, b, f'job {j}: {f}')
    assert all(torch.isfinite(v).all() for v in fp['agent.pth']['actor'].values())
    jobs.append(fp)
  for i in range(len(seeds)):   # every pair: two later jobs that came out equal (one seed wired to both) must not pass
    for j in range(i + 1, len(seeds)):
      assert any(not torch.equal(v, jobs[j]['agent.pth']['actor'][k]) for k, v in jobs[i]['agent.pth']['actor'].items()), f'jobs {i} and {j}: the jobs of a seed sweep are meant to differ'
      assert jobs[i]['metrics.pth']['test_returns'] != jobs[j]['metrics.pth']['test_returns'], f'jobs {i} and {j}'


@pytest.mark.parametrize('args', [['algorithm=GAIL', 'env=hopper'], ['algorithm=SAC', 'env=walker2d', '+acting.schedule=fused']], ids=['GAIL-hopper-exact', 'SAC-walker2d-fused'])
def test_seed_sweep_population_equals_per_learner(tmp_path, args):
  sweep_schedules_leave_the_same_bytes(tmp_path, args, (3, 4, 5), COMMON)


def test_seed_sweep_with_pugail_loss_and_bc_pretraining_equals_per_learner(tmp_path):
  """A GAIL loss other than BCE (PUGAIL, infinite margin) and `bc_pretraining.iterations > 0` (one PretrainPlan per learner in front of the loop) under both schedules."""
  sweep_schedules_leave_the_same_bytes(tmp_path, ['algorithm=GAIL', 'env=hopper', 'imitation.loss_function=PUGAIL', 'bc_pretraining.iterations=20'], (3, 4), COMMON)


def test_seed_sweep_graph_replays_equal_direct_launches(tmp_path, monkeypatch, short=None):
  """IL_TRAIN_LAUNCH=graph captures the population update after its first, eager, run and replays it: the same bytes as the direct launches."""
  argv = ['-m', 'seed=3,4', 'algorithm=GAIL', 'env=hopper', '+sweep.schedule=population'] + (short or COMMON)
  monkeypatch.setenv('IL_TRAIN_LAUNCH', 'direct')
  root_d, scores_d = _sweep(tmp_path, 'direct', argv)
  monkeypatch.setenv('IL_TRAIN_LAUNCH', 'graph')
  root_g, scores_g = _sweep(tmp_path, 'graph', argv)
  assert np.isfinite(scores_d).all() and scores_d == scores_g
  for j in (0, 1):
    fd, fg = _job_files(root_d, j), _job_files(root_g, j)
    assert set(fd) == set(fg) == {'agent.pth', 'discriminator.pth', 'metrics.pth'}
    for f in fd:
      a, b = ({k: v for k, v in m.items() if k not in TIMING_KEYS} for m in (fd[f], fg[f]))
      _assert_same_nested(a, b, f'job {j}: {f}')


def test_sweep_without_population_launches_runs_job_after_job(tmp_path, capsys):
  """PWIL has no population launches: the sweep runs its jobs one after another through train(), says so on stderr, and leaves two job directories."""
  root, scores = _sweep(tmp_path, 'pwil', ['-m', 'seed=1,2', 'algorithm=PWIL', 'env=walker2d'] + COMMON)
  err = capsys.readouterr().err
  assert err.count('[train] sweep:') == 2 and 'one job after another' in err and 'algorithm=PWIL has no population launches' in err
  assert sorted(os.listdir(root)) == ['0', '1'] and np.isfinite(scores).all()
  for j in (0, 1):
    assert {'agent.pth', 'metrics.pth'} <= set(os.listdir(os.path.join(root, str(j))))
