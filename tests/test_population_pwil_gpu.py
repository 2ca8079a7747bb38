"""`-m gpu`: PWIL seed sweeps as one population - the coupling launch for L learners (`il_pwil_act_reward_population`: k_pwil_couple_population, grid (chunk, learner))
in front of `il_act_step_population`, through `il.PopulationActingWorker(reward_models=...)`, and `python train.py -m seed=... algorithm=PWIL +sweep.pwil_population=true`.

The oracle of the launch is the per-learner path, one `il.ActingWorker(reward_model=...)` per learner (`il_pwil_act_reward` + `il_act_step`), bit for bit: actions, whole
rings with their reward columns, atom weights, carries, cursors. The learners' atom sets differ in size (600, 520 and 257 atoms: rows of 3, 3 and 2 chunks in a grid 3
wide, the last chunk of the third holding one atom), their episodes end at different steps, and now and then one of them idles. The reward columns are also held against
the numpy oracle at the bound of the other PWIL parity tests (rtol 2e-5). The bodies also run on the host emulation of the kernels
(tests/test_population_pwil_emulated.py), whose workgroups do not run in lockstep."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import inputs as gi
from oracle import pwil as opwil

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib
  from gpu_util import DEV, N, Cfg

import test_population_acting_gpu as tpa   # _learner_script, _Lockstep, _sweep, _job_files (names looked up at call time: the emulated file rebinds that module's il / DEV)
import test_pwil_acting_gpu as tpw         # _discriminator, PWIL_CFG
from test_train_gpu import COMMON          # (the short step counts of tests/test_train_gpu.py)

ATOMS, HORIZON = (600, 520, 257), 40       # m = 17, 15, 9 candidates per chunk over G = 3, 3, 2 chunks
CAPACITY, STEPS, BOGUS = 37, 60, 1e9       # a 37-row ring wraps under 60 steps; the reward argument is the caller's and must never reach the ring
IDLE = {1: (12, 13), 2: (33,)}             # learner: the lockstep launches in which it idles (learner 0 never does)
SEEDS = (1000, 1017, 1034)


def _ticket(disc):
  return int(N(disc._dists)[-4:].view(np.uint32)[0])


def _scripts(S, absorbing):
  """tests/test_population_acting_gpu.py's per-learner scripts (true terminations at 7 + l, 31 + l, 52 + l, timeouts at 19 + l, 44 + l: one learner's device-side reset
  happens while the others are mid-episode), with a reward argument that would show in the ring."""
  out = []
  for l in range(len(ATOMS)):
    script, first, resets = tpa._learner_script(l, STEPS, S, absorbing)
    out.append(([(o, BOGUS, te, to) for o, _, te, to in script], first, resets))
  return out


def _population(env, absorbing):
  """L actors (own parameters), empty rings and discriminators on learner l's own atoms (gi.pwil_case under a seed of its own)."""
  S, A = gi.DIMS[env]
  actors, _, mems, _ = tpa._actors_and_memories(S, A, 64, len(ATOMS), absorbing, capacity=CAPACITY)
  atoms = [gi.pwil_case(41 + l, n, S + A, 1)[0] for l, n in enumerate(ATOMS)]
  discs = [tpw._discriminator(a, S, HORIZON)[0] for a in atoms]
  for d, n in zip(discs, ATOMS):
    m, G = int(np.ceil((1 / HORIZON - 1e-6) * n)) + 2, -(-n // 256)
    assert (n, m, G) in ((600, 17, 3), (520, 15, 3), (257, 9, 2)) and d.expert_atoms.size(0) == n
  return actors, mems, discs, atoms


_REFERENCE, _ORACLE = {}, {}   # the per-learner side once per (device, env, absorbing, schedule); the oracle's reward columns once per (env, absorbing): never written again


def _reference(env, absorbing, schedule):
  """One ActingWorker(reward_model=...) per learner through its script. The population's commit sequence advances once per launch for all learners, also while one of
  them idles; the reference worker's sequence is advanced over those launches (two posts per launch under the exact schedule, one under the fused), so that the commit
  words in the carries compare exactly too."""
  key = (str(DEV), env, absorbing, schedule)
  if key in _REFERENCE: return _REFERENCE[key]
  S, A = gi.DIMS[env]
  actors, mems, discs, atoms = _population(env, absorbing)
  scripts, out = _scripts(S, absorbing), []
  for l, (script, first, resets) in enumerate(scripts):
    w = il.ActingWorker(actors[l], mems[l], reward_model=discs[l], noise_seed=SEEDS[l])
    acts, k, t, launch = [], 0, 0, 0
    obs = first
    a = w.act(first) if schedule == 'fused' else None
    while t < STEPS:
      launch += 1
      if launch in IDLE.get(l, ()):
        for _ in range(2 if schedule == 'exact' else 1): w._next_seq()
        continue
      nxt, rew, term, tout = script[t]
      t += 1
      ended = term or tout
      if schedule == 'exact':
        acts.append(N(w.act(obs)))
        w.append(t, nxt, rew, term, tout)
        obs = resets[k] if ended else nxt
      else:
        acts.append(N(a))
        a = w.step(t, nxt, rew, term, tout, obs=resets[k] if ended else None)
      k += int(ended)
    torch.cuda.synchronize()
    assert mems[l].full, 'the script is meant to wrap the ring'
    out.append(dict(actions=np.concatenate(acts), ring=N(mems[l].ring), weights=N(discs[l].expert_weights), carry=N(w.carry), ring_state=N(mems[l]._ring_state),
                    host=(mems[l].idx, mems[l].full, mems[l].num_trajectories), act_calls=actors[l]._act_calls, ticket=_ticket(discs[l])))
  _REFERENCE[key] = out
  return out


def _oracle_rewards(env, absorbing, actions):
  """The numpy oracle's reward column of every learner's ring for the actions the device took: the row each step is stored in (later steps overwrite earlier rows of the
  wrapped ring), zero in the absorbing -> absorbing row behind a true termination."""
  key = (env, absorbing)
  if key in _ORACLE: return _ORACLE[key]
  S, A = gi.DIMS[env]
  out = []
  for l, n in enumerate(ATOMS):
    atoms = gi.pwil_case(41 + l, n, S + A, 1)[0]
    oracle = opwil.PwilOracle(atoms, HORIZON, tpw.PWIL_CFG['reward_scale'], tpw.PWIL_CFG['reward_bandwidth_scale'])
    script, first, resets = _scripts(S, absorbing)[l]
    want, cursor, obs, k = np.zeros(CAPACITY), 0, first, 0
    for t, (nxt, _, term, tout) in enumerate(script):
      want[cursor % CAPACITY] = oracle.compute_reward(np.concatenate([obs, actions[l][t]]))
      cursor += 1
      if term or tout:
        if absorbing and term and not tout:
          want[cursor % CAPACITY] = 0.0
          cursor += 1
        oracle.reset()
        obs = resets[k]; k += 1
      else:
        obs = nxt
    out.append(want)
  _ORACLE[key] = out
  return out


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
@pytest.mark.parametrize('env', ['hopper', 'halfcheetah'])
def test_population_pwil_matches_per_learner_workers(env, schedule, absorbing):
  """60 steps per learner into rings of 37 rows, L = 3 learners on 600 / 520 / 257 atoms at horizon 40; hopper: D = 15, the scalar distance loop, halfcheetah: D = 24,
  the 16-byte-lane loop. Per learner, exactly: actions, the whole ring with its reward column, the atom weights, the carry (state | action, consumed word, reward, coupled
  word), the device cursor and the host mirrors; every arrival ticket ends at zero; the reward column is within rtol 2e-5 of the numpy oracle."""
  S, A = gi.DIMS[env]
  assert (S + A) % 4 == (3 if env == 'hopper' else 0)
  ref = _reference(env, absorbing, schedule)
  actors, mems, discs, _ = _population(env, absorbing)
  w = il.PopulationActingWorker(actors, mems, SEEDS, reward_models=discs)
  run = tpa._Lockstep(w, schedule, _scripts(S, absorbing))
  launch = 0
  while min(run.t) < STEPS:
    launch += 1
    run.launch([l for l in range(w.L) if run.t[l] < STEPS and launch not in IDLE.get(l, ())])
  torch.cuda.synchronize()
  assert launch == STEPS + 2 and run.t == [STEPS] * w.L
  for l in range(w.L):
    r, what = ref[l], f'learner {l}'
    np.testing.assert_array_equal(r['actions'], run.actions(l), err_msg=what)
    np.testing.assert_array_equal(r['ring'], N(mems[l].ring), err_msg=what)
    np.testing.assert_array_equal(r['weights'], N(discs[l].expert_weights), err_msg=what)
    np.testing.assert_array_equal(r['carry'].view(np.uint32), N(w.carry[l]).view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(r['ring_state'], N(mems[l]._ring_state), err_msg=what)
    assert r['host'] == (mems[l].idx, mems[l].full, mems[l].num_trajectories) and N(mems[l]._ring_state).tolist() == [mems[l].idx, int(mems[l].full), mems[l].size], what
    assert r['act_calls'] == actors[l]._act_calls, what
    assert r['ticket'] == 0 and _ticket(discs[l]) == 0, f'{what}: the arrival ticket must end at zero'
  want = _oracle_rewards(env, absorbing, [r['actions'] for r in ref])
  for l in range(w.L):
    rewards = N(mems[l].ring)[:, 2 * S + A]
    assert not (rewards == np.float32(BOGUS)).any() and (rewards != 0).sum() >= 30
    np.testing.assert_allclose(rewards, want[l], rtol=2e-5, err_msg=f'learner {l}')
  assert not np.array_equal(N(mems[0].ring), N(mems[1].ring)), 'the learners are meant to differ'


def _state(w, mems, discs):
  torch.cuda.synchronize()
  return [N(w.carry).copy()] + [N(d.expert_weights).copy() for d in discs] + [N(m.ring).copy() for m in mems] + [N(m._ring_state).copy() for m in mems] + [np.array([_ticket(d) for d in discs])]


def _assert_unchanged(before, after, what):
  for i, (a, b) in enumerate(zip(before, after)):
    np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b, err_msg=f'{what} (array {i})')


@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_population_pwil_idle_and_replayed_launches_change_nothing(schedule):
  """The coupling (with the acting launch behind it) issued a second time without a new post - mid-episode, with atom weights partly consumed, and right behind a true
  termination and a timeout - and a post in which every learner idles: atom weights, carries, rings, cursors and tickets keep their bits."""
  env, absorbing = 'hopper', True
  S, A = gi.DIMS[env]
  actors, mems, discs, _ = _population(env, absorbing)
  w = il.PopulationActingWorker(actors, mems, SEEDS, reward_models=discs)
  run = tpa._Lockstep(w, schedule, _scripts(S, absorbing))
  every, box = list(range(w.L)), (w._append_box if schedule == 'exact' else w._act_box)
  L = _lib.lib()
  for launch in range(1, 22):
    run.launch(every)
    if launch in (5, 7, 8, 9, 19, 21):   # 7, 8, 9: the true terminations of learners 0, 1, 2; 19, 21: timeouts of learners 0 and 2; 5: everybody mid-episode
      before = _state(w, mems, discs)
      if launch == 5:
        assert all((b < np.float32(1 / n)).any() for b, n in zip(before[1:4], ATOMS)), 'mid-episode: atoms are meant to be partly consumed'
      _lib.check(L.il_pwil_act_reward_population(_lib.ptr(w._pwil_descs[id(box)]), w.L, C.byref(w._pwil_shape), _lib.stream_ptr()))   # the coupling alone ...
      _assert_unchanged(before, _state(w, mems, discs), f'launch {launch}: a coupling replayed without a new post')
      w._launch(box, appends=True)                                                                                                     # ... and the pair
      _assert_unchanged(before, _state(w, mems, discs), f'launch {launch}: a coupling + acting pair replayed without a new post')
  before = _state(w, mems, discs)
  run.launch([])   # a post in which every learner idles
  _assert_unchanged(before, _state(w, mems, discs), 'a post in which every learner idles')
  assert before[-1].tolist() == [0, 0, 0]
  run.launch(every)   # and the population goes on
  after = _state(w, mems, discs)
  assert all(not np.array_equal(a, b) for a, b in zip(before[4:7], after[4:7])), 'every ring takes the next transition'


def test_population_pwil_uncoupled_post_is_left_alone():
  """A post whose learners all carry PENDING | REWARD_ON_DEVICE, a coupling launch for learners 0 and 2 only, then il_act_step_population for all three: learner 1 - no
  coupling in front of its append - gets no row, no cursor move and no echo; the other two are appended. The pair enqueued behind it then appends learner 1 with the
  reward of its own coupling and leaves the other two alone. Raw launches and torch.cuda.synchronize(), as the overlap body of tests/test_pwil_acting_gpu.py."""
  from imitation_learning_amd.acting import NO_ACTION, PENDING, REWARD_ON_DEVICE
  from imitation_learning_amd.training import _device_array
  env, absorbing = 'hopper', True
  S, A = gi.DIMS[env]
  actors, mems, discs, _ = _population(env, absorbing)
  w = il.PopulationActingWorker(actors, mems, SEEDS, reward_models=discs)
  scripts = _scripts(S, absorbing)
  w.act([s[1] for s in scripts])
  box, every = w._append_box, [0, 1, 2]
  rows, wrap, flags = w._transition_flags([s[0][0][0] for s in scripts], [False] * 3, [False] * 3)
  assert (flags == PENDING | REWARD_ON_DEVICE).all()
  flags |= NO_ACTION
  w._post_transition(box, rows, 1, [s[0][0][0] for s in scripts], [BOGUS] * 3, [False] * 3, [False] * 3)
  words = box.commit(w._next_seq(), flags).copy()
  base, stride = box.tensor.data_ptr(), box.floats * 4
  two = _device_array([_lib.PwilLearner(discs[l]._desc, base + l * stride, w.carry[l].data_ptr()) for l in (0, 2)], w.device)
  L = _lib.lib()
  before = _state(w, mems, discs)
  _lib.check(L.il_pwil_act_reward_population(_lib.ptr(two), 2, C.byref(w._pwil_shape), _lib.stream_ptr()))
  _lib.check(L.il_act_step_population(_lib.ptr(w._descs[id(box)]), 3, S, A, w.H, _lib.stream_ptr()))
  after = _state(w, mems, discs)
  col = 2 * S + A
  for l in (0, 2):
    assert after[7 + l].tolist() == [1, 0, CAPACITY] and float(box.echo[l]) == words[l], f'learner {l}: coupled and appended'
    assert after[4 + l][0, col] not in (0.0, np.float32(BOGUS)) and not np.array_equal(before[1 + l], after[1 + l])
  np.testing.assert_array_equal(before[4 + 1], after[4 + 1], err_msg='learner 1: a post without its coupling got a row')
  np.testing.assert_array_equal(before[1 + 1], after[1 + 1]); np.testing.assert_array_equal(before[0][1].view(np.uint32), after[0][1].view(np.uint32))
  assert after[7 + 1].tolist() == [0, 0, CAPACITY] and float(box.echo[1]) != words[1], 'learner 1: no cursor move and no echo'
  w._launch(box, appends=True)   # the pair behind the post
  w._append_launched = True
  last = _state(w, mems, discs)
  assert last[7 + 1].tolist() == [1, 0, CAPACITY] and float(box.echo[1]) == words[1] and last[4 + 1][0, col] not in (0.0, np.float32(BOGUS))
  for l in (0, 2):
    for i in (1 + l, 4 + l, 7 + l): np.testing.assert_array_equal(after[i], last[i], err_msg=f'learner {l}: appended or coupled twice')
  assert last[-1].tolist() == [0, 0, 0]
  w._mirror_appends(every, [False] * 3, [False] * 3, wrap)   # the host mirrors of the three appends
  # learner 1's row is the one its own ActingWorker stores for that transition
  ref_actors, ref_mems, ref_discs, _ = _population(env, absorbing)
  single = il.ActingWorker(ref_actors[1], ref_mems[1], reward_model=ref_discs[1], noise_seed=SEEDS[1])
  single.act(scripts[1][1]); single.append(1, scripts[1][0][0][0], BOGUS, False, False)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(N(ref_mems[1].ring), last[4 + 1]); np.testing.assert_array_equal(N(ref_discs[1].expert_weights), last[1 + 1])


def test_population_pwil_learner_wider_than_the_grid_is_not_coupled():
  """shape_host is meant to be the largest learner's descriptor. Given the smallest one's (257 atoms: a grid 2 chunks wide), the learners of 3 chunks are not coupled at
  all - no weight or carry word moves, their tickets stay at zero, and the appending launch leaves their posts alone - while the learner that fits is coupled and appended;
  the pair with the right shape then appends the other two."""
  from imitation_learning_amd.acting import NO_ACTION
  env, absorbing = 'hopper', True
  S, A = gi.DIMS[env]
  actors, mems, discs, _ = _population(env, absorbing)
  w = il.PopulationActingWorker(actors, mems, SEEDS, reward_models=discs)
  scripts = _scripts(S, absorbing)
  w.act([s[1] for s in scripts])
  box = w._append_box
  nxt = [s[0][0][0] for s in scripts]
  rows, wrap, flags = w._transition_flags(nxt, [False] * 3, [False] * 3)
  w._post_transition(box, rows, 1, nxt, [BOGUS] * 3, [False] * 3, [False] * 3)
  words = box.commit(w._next_seq(), flags | NO_ACTION).copy()
  L = _lib.lib()
  before = _state(w, mems, discs)
  _lib.check(L.il_pwil_act_reward_population(_lib.ptr(w._pwil_descs[id(box)]), 3, C.byref(discs[2]._desc), _lib.stream_ptr()))
  _lib.check(L.il_act_step_population(_lib.ptr(w._descs[id(box)]), 3, S, A, w.H, _lib.stream_ptr()))
  after = _state(w, mems, discs)
  for l in (0, 1):
    for i in (1 + l, 4 + l, 7 + l): np.testing.assert_array_equal(before[i], after[i], err_msg=f'learner {l}: wider than the grid, yet something of it moved')
    np.testing.assert_array_equal(before[0][l].view(np.uint32), after[0][l].view(np.uint32))
    assert float(box.echo[l]) != words[l]
  assert after[7 + 2].tolist() == [1, 0, CAPACITY] and float(box.echo[2]) == words[2] and after[-1].tolist() == [0, 0, 0]
  w._launch(box, appends=True)
  w._append_launched = True
  last = _state(w, mems, discs)
  assert all(last[7 + l].tolist() == [1, 0, CAPACITY] and float(box.echo[l]) == words[l] for l in range(3)) and last[-1].tolist() == [0, 0, 0]
  for i in (1 + 2, 4 + 2, 7 + 2): np.testing.assert_array_equal(after[i], last[i], err_msg='learner 2: appended or coupled twice')
  w._mirror_appends([0, 1, 2], [False] * 3, [False] * 3, wrap)


def _shape_desc(n, horizon, S, A, buf):
  p = buf.data_ptr()
  return _lib.Pwil(n, S + A, S, A, p, p, p, p, p, 5.0, 1.0, 1 / horizon - 1e-6)


def test_population_pwil_loud_failures():
  """Refused before anything is launched, each naming the function: null descriptors, no learners, more learners than the grid's y axis holds, and a shape outside the
  one-launch coupling (with its limits). And the worker's refusals."""
  S, A = gi.DIMS['hopper']
  L = _lib.lib()
  buf = torch.zeros(4096, device=DEV)
  ok = _shape_desc(600, 40, S, A, buf)
  arg, unsupported = 1, 2   # IL_ERR_ARG, IL_ERR_UNSUPPORTED (include/il_hip.h)
  for args, rc, words in (((None, 3, C.byref(ok), None), arg, [b'null']), ((_lib.ptr(buf), 3, None, None), arg, [b'null']), ((_lib.ptr(buf), 0, C.byref(ok), None), arg, [b'n_learners=0', b'65535']),
                          ((_lib.ptr(buf), 65536, C.byref(ok), None), arg, [b'n_learners=65536', b'65535']),
                          ((_lib.ptr(buf), 3, C.byref(_shape_desc(3000, 10, S, A, buf)), None), unsupported, [b'<= 256', b'<= 4096', b'n_atoms=3000']),
                          ((_lib.ptr(buf), 3, C.byref(_shape_desc(6000, 30, S, A, buf)), None), unsupported, [b'<= 256', b'<= 4096', b'n_atoms=6000'])):
    assert L.il_pwil_act_reward_population(*args) == rc, args
    err = L.il_last_error()
    assert b'il_pwil_act_reward_population' in err and all(x in err for x in words), err
  torch.cuda.synchronize()
  assert not N(buf).any()

  actors, mems, discs, atoms = _population('hopper', True)
  with pytest.raises(ValueError, match='mixes None'):
    il.PopulationActingWorker(actors, mems, SEEDS, reward_models=[discs[0], None, discs[2]])
  with pytest.raises(ValueError, match='per learner'):
    il.PopulationActingWorker(actors, mems, SEEDS, reward_models=discs[:2])
  other_horizon = tpw._discriminator(atoms[1], S, HORIZON + 1)[0]
  with pytest.raises(ValueError, match='time_horizon'):
    il.PopulationActingWorker(actors, mems, SEEDS, reward_models=[discs[0], other_horizon, discs[2]])
  state_only = il.PWILDiscriminator(S, A, Cfg(**dict(tpw.PWIL_CFG, state_only=True)), tpw._expert(atoms[1], S), HORIZON)
  with pytest.raises(ValueError, match='state_only'):
    il.PopulationActingWorker(actors, mems, SEEDS, reward_models=[discs[0], state_only, discs[2]])

  class Reward:   # not a PWIL reward model
    pass
  with pytest.raises(NotImplementedError, match='PWIL'):
    il.PopulationActingWorker(actors, mems, SEEDS, reward_models=[Reward(), Reward(), Reward()])
  big = tpw._discriminator(gi.pwil_case(47, 8000, S + A, 1)[0], S, HORIZON)[0]   # m = 202 over 32 chunks: il_pwil_reward's two-launch size
  with pytest.raises(NotImplementedError, match='<= 256.*<= 4096'):
    il.PopulationActingWorker(actors, mems, SEEDS, reward_models=[discs[0], big, discs[2]])
  il.PopulationActingWorker(actors, mems, SEEDS, reward_models=[None, None, None])   # no reward model at all: the plain population worker
  plain = il.PopulationActingWorker(actors, mems, SEEDS)
  assert plain.reward_models is None and plain._reward_flag == 0


# ------------------------------------------------------------------------------------------------ train.py -m
PWIL_RUN = ['algorithm=PWIL', 'env=walker2d']
KEY = '+sweep.pwil_population=true'


def _single(tmp_path, name, seed, extra, short):
  """One train.py run of one seed in its own directory, from fresh process-wide update counters."""
  if ROOT not in sys.path: sys.path.insert(0, ROOT)
  import train
  from imitation_learning_amd import config, training as il_training
  il_training._NOISE.clear(); il_training._WS.clear()
  d = tmp_path / name
  d.mkdir()
  before = os.getcwd()
  os.chdir(d)
  try:
    train.train(config.compose(PWIL_RUN + [f'seed={seed}'] + list(extra) + short))
  finally:
    os.chdir(before)
  return {f: torch.load(d / f, weights_only=False) for f in ('agent.pth', 'metrics.pth')}


def _same_job(a, b, what):
  for part in ('actor', 'critic'):
    tpa._assert_same_nested(a['agent.pth'][part], b['agent.pth'][part], f'{what}: {part}')
  tpa._assert_same_nested(a['agent.pth']['log_alpha'], b['agent.pth']['log_alpha'], f'{what}: log_alpha')
  for key in ('train_returns', 'predicted_rewards'):
    tpa._assert_same_nested(a['metrics.pth'][key], b['metrics.pth'][key], f'{what}: {key}')


@pytest.mark.parametrize('extra', [[], ['imitation.mix_expert_data=prefill_memory']], ids=['none', 'prefill_memory'])
def test_pwil_seed_sweep_population_equals_per_learner_equals_single_runs(tmp_path, capsys, extra, short=None):
  """`-m seed=1,2 algorithm=PWIL env=walker2d +sweep.pwil_population=true` under +sweep.schedule=population, under per_learner and as two single train() runs: the learner
  (actor, critic, log_alpha) and the train_returns / predicted_rewards metrics bit for bit the same three times; each sweep announces one population of 2 learners and
  saves no discriminator.pth. prefill_memory: every learner relabels its own expert memory on the device and moves it into its ring in front of the loop."""
  short = short or COMMON
  argv = ['-m', 'seed=1,2'] + PWIL_RUN + [KEY] + extra + short
  jobs = {}
  for schedule in ('population', 'per_learner'):
    capsys.readouterr()
    root, scores = tpa._sweep(tmp_path, schedule, argv + [f'+sweep.schedule={schedule}'])
    err = capsys.readouterr().err
    assert err.count('[train] sweep:') == 1 and err.count('one population of 2 learners') == 1 and f'+sweep.schedule={schedule}' in err, err
    assert np.isfinite(scores).all() and sorted(os.listdir(root)) == ['0', '1']
    jobs[schedule] = [tpa._job_files(root, j) for j in (0, 1)]
    assert all(set(f) == {'agent.pth', 'metrics.pth'} for f in jobs[schedule]), 'train_sweep saves no discriminator.pth for PWIL, as train()'
  singles = [_single(tmp_path, f'single{seed}', seed, extra, short) for seed in (1, 2)]
  for j in (0, 1):
    m = jobs['population'][j]['metrics.pth']
    assert len(m['update_steps']) >= 2 and len(m['train_returns']) >= 2 and all(np.isfinite(r).all() and (r >= 0).all() for r in m['predicted_rewards'])
    _same_job(jobs['population'][j], jobs['per_learner'][j], f'job {j}: population against per_learner')
    _same_job(jobs['population'][j], singles[j], f'job {j}: the sweep against a single run of seed {j + 1}')
  a0, a1 = (jobs['population'][j]['agent.pth']['actor'] for j in (0, 1))
  assert any(not torch.equal(v, a1[k]) for k, v in a0.items()), 'the jobs of a seed sweep are meant to differ'
