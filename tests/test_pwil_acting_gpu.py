"""`-m gpu`: PWIL through the acting worker (`ActingWorker(reward_model=PWILDiscriminator)`: `il_pwil_act_reward` in front of every appending launch, the append
storing the reward from the carry under IL_ACT_REWARD_ON_DEVICE) and the device-resident expert relabel (`PWILDiscriminator.relabel_memory`: `il_pwil_relabel_rows`).

Both must leave what train.py's per-function sequence leaves - `actor(obs).sample()`, `compute_reward(...)` with its `.item()`, `memory.append`,
`wrap_for_absorbing_states`, `reset()` at episode ends - bit for bit: the actions, the whole ring with its reward column, the atom weights. The reward column is
also held against the numpy oracle at the bound of the other PWIL parity tests (rtol 2e-5). The bodies also run on the host emulation of the kernels
(tests/test_pwil_acting_emulated.py), whose workgroups do not run in lockstep and whose graph replays are real replays."""
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

from test_gpu_parity import _episode_script
from test_train_gpu import COMMON   # (the short step counts of tests/test_train_gpu.py)

PWIL_CFG = dict(state_only=False, reward_scale=5, reward_bandwidth_scale=5)
ATOMS = {'n600_t40': (600, 40), 'n2000_t100': (2000, 100)}   # (atoms, time horizon): m = 17 candidates per chunk over G = 3 chunks; m = 22 over G = 8
# name: (hidden, depth, activation) at Hopper dims. The shipped shape takes il_act_step; the other two il_act_step_general in its one-launch form (a) and in its
# layer-at-a-time form (b), whose commit kernel does the append
ACTORS = {'shipped_h64': (64, 2, 'relu'), 'd3_tanh_h48_hopper': (48, 3, 'tanh'), 'h50_d2_relu_hopper': (50, 2, 'relu')}


def _expert(atoms, S, ends=None):
  """An expert ReplayMemory whose (state | action) rows are `atoms`; `ends`: {row: 'terminals' | 'timeouts'}."""
  n = atoms.shape[0]
  flags = dict(terminals=torch.zeros(n), timeouts=torch.zeros(n))
  for row, kind in (ends or {}).items(): flags[kind][row] = 1.0
  A = atoms.shape[1] - S
  return il.ReplayMemory(n, S, A, False, transitions=dict(states=torch.from_numpy(atoms[:, :S]), actions=torch.from_numpy(atoms[:, S:]), rewards=torch.zeros(n),
                                                          next_states=torch.from_numpy(atoms[:, :S]), weights=torch.ones(n), num_trajectories=4, **flags), device=DEV)


def _discriminator(atoms, S, horizon, ends=None):
  mem = _expert(atoms, S, ends)
  return il.PWILDiscriminator(S, atoms.shape[1] - S, Cfg(**PWIL_CFG), mem, horizon), mem


def _actor(S, A, H, depth, activation):
  torch.manual_seed(3)
  actor = il.SoftActor(S, A, Cfg(hidden_size=H, depth=depth, activation=activation), device=DEV)
  actor.flat.copy_(torch.randn_like(actor.flat) * 0.08)
  return actor


def _script(S, absorbing):
  rs = np.random.RandomState(5)
  script = _episode_script(rs, 60, S, absorbing)   # true terminations at steps 7, 31, 52, timeouts at 19, 44: five device-side resets
  first = rs.standard_normal(S).astype(np.float32); first[-1] = 0.0 if absorbing else first[-1]
  resets = [rs.standard_normal(S).astype(np.float32) * 0.1 for _ in range(8)]
  if absorbing:
    for r in resets: r[-1] = 0.0
  return script, first, resets


_SIDE_A = {}   # the per-function side and the oracle's rewards, once per (device, actor, atoms, absorbing): every schedule is compared with the same arrays


def _per_function_side(actor_name, atoms_name, absorbing):
  key = (str(DEV), actor_name, atoms_name, absorbing)
  if key in _SIDE_A: return _SIDE_A[key]
  S, A = gi.DIMS['hopper']
  n, horizon = ATOMS[atoms_name]
  atoms, _ = gi.pwil_case(41, n, S + A, 1)
  actor, (disc, _), mem = _actor(S, A, *ACTORS[actor_name]), _discriminator(atoms, S, horizon), il.ReplayMemory(37, S, A, absorbing, device=DEV)
  oracle = opwil.PwilOracle(atoms, horizon, PWIL_CFG['reward_scale'], PWIL_CFG['reward_bandwidth_scale'])
  script, first, resets = _script(S, absorbing)
  acts, want, obs, k = [], np.zeros(37), torch.from_numpy(first).unsqueeze(0), 0
  for t, (nxt, rew, term, tout) in enumerate(script, 1):   # train.py's per-function loop
    a = actor(obs).sample()
    acts.append(N(a))
    reward = disc.compute_reward(obs, a)
    want[mem.idx] = oracle.compute_reward(np.concatenate([N(obs)[0], acts[-1][0]]))   # the oracle's reward column: the row this step is stored in ...
    nxt_t = torch.from_numpy(nxt).unsqueeze(0)
    mem.append(t, obs, a, reward, nxt_t, term, tout)
    if term or tout:
      if absorbing and term and not tout:
        want[mem.idx] = 0.0   # ... and the absorbing -> absorbing row behind it
        mem.wrap_for_absorbing_states()
      disc.reset(); oracle.reset()
      obs = torch.from_numpy(resets[k]).unsqueeze(0); k += 1
    else:
      obs = nxt_t
  torch.cuda.synchronize()
  assert mem.full, 'the script is meant to wrap the ring'
  out = _SIDE_A[key] = dict(actions=np.concatenate(acts), ring=N(mem.ring), weights=N(disc.expert_weights), host=(mem.idx, mem.full, mem.num_trajectories), oracle_rewards=want, atoms=atoms)
  return out


def _worker_matches_separate_calls(actor_name, atoms_name, absorbing, schedule):
  a_side = _per_function_side(actor_name, atoms_name, absorbing)
  S, A = gi.DIMS['hopper']
  n, horizon = ATOMS[atoms_name]
  actor, (disc, _), mem = _actor(S, A, *ACTORS[actor_name]), _discriminator(a_side['atoms'], S, horizon), il.ReplayMemory(37, S, A, absorbing, device=DEV)
  m, G = int(np.ceil((1 / horizon - 1e-6) * n)) + 2, -(-n // 256)
  assert (m, G) == {'n600_t40': (17, 3), 'n2000_t100': (22, 8)}[atoms_name]
  script, first, resets = _script(S, absorbing)
  w = il.ActingWorker(actor, mem, mirror=schedule == 'overlap', reward_model=disc)
  acts, k = [], 0
  bogus = 1e9   # the reward argument is the caller's (train_return): with a reward model it must not reach the ring
  if schedule == 'exact':
    obs = first
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts.append(N(w.act(obs)))
      w.append(t, nxt, bogus, term, tout)
      if term or tout: obs = resets[k]; k += 1
      else: obs = nxt
  elif schedule == 'fused':
    a = w.act(first)
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts.append(N(a))
      ended = term or tout
      a = w.step(t, nxt, bogus, term, tout, obs=resets[k] if ended else None)
      k += int(ended)
  else:
    obs, a = first, w.act(first)
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts.append(N(a))
      if t in (10, 44, 52):   # a replayed pair still in flight as the host posts again - mid-episode, at a timeout, at a true termination: its coupling runs before the post ...
        box = w._append_box
        _lib.check(_lib.lib().il_pwil_act_reward(C.byref(disc._desc), C.c_void_p(box.tensor.data_ptr()), _lib.ptr(w.carry), _lib.stream_ptr()))
        torch.cuda.synchronize()
        before = N(mem.ring), N(disc.expert_weights), N(mem._ring_state), float(box.host[box.o_echo])
        w.post(t, obs, a, nxt, bogus, term, tout)
        w._launch(box, acts=False)   # ... and its append after it: it must neither store the previous transition's reward for this post nor echo it
        torch.cuda.synchronize()
        np.testing.assert_array_equal(N(mem.ring), before[0], err_msg=f'step {t}: a post was appended without its coupling')
        np.testing.assert_array_equal(N(disc.expert_weights), before[1]); np.testing.assert_array_equal(N(mem._ring_state), before[2])
        assert float(box.host[box.o_echo]) == before[3] != box.word, f'step {t}: an append that left the post alone must not echo it'
      else:
        w.post(t, obs, a, nxt, bogus, term, tout)
      w.enqueue_append()   # the pair enqueued behind the post
      if t in (3, 19, 25, 31):   # an append without a new post - mid-episode, and right behind both kinds of episode end: nothing may be coupled, reset or appended twice
        torch.cuda.synchronize()
        before = N(mem.ring), N(disc.expert_weights)
        w.enqueue_append()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(N(mem.ring), before[0], err_msg=f'ring changed by a replayed append at step {t}')
        np.testing.assert_array_equal(N(disc.expert_weights), before[1], err_msg=f'atom weights changed by a replayed coupling at step {t}')
      ended = term or tout
      obs = resets[k] if ended else nxt
      k += int(ended)
      a = w.act(obs)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(a_side['actions'], np.concatenate(acts))
  ring = N(mem.ring)
  np.testing.assert_array_equal(a_side['ring'], ring)
  np.testing.assert_array_equal(a_side['weights'], N(disc.expert_weights))
  assert a_side['host'] == (mem.idx, mem.full, mem.num_trajectories)
  assert N(mem._ring_state).tolist() == [mem.idx, int(mem.full), mem.size]
  assert int(N(disc._dists)[-4:].view(np.uint32)[0]) == 0, 'the arrival ticket must end at zero'
  rewards = ring[:, 2 * S + A]
  assert not (rewards == np.float32(bogus)).any() and (rewards != 0).sum() >= 30
  np.testing.assert_allclose(rewards, a_side['oracle_rewards'], rtol=2e-5)


@pytest.mark.parametrize('atoms', list(ATOMS))
@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('schedule', ['exact', 'fused', 'overlap'])
def test_pwil_worker_matches_separate_calls(schedule, absorbing, atoms):
  """60 steps into a ring of 37 rows with three true terminations and two timeouts, shipped actor shape: actions, ring (reward column included), atom weights and the
  host's cursor / full / trajectory count equal to the per-function sequence's; the reward column within rtol 2e-5 of the oracle. n2000_t100 spreads the select over
  eight workgroups, so the last arriver is not always the same one."""
  _worker_matches_separate_calls('shipped_h64', atoms, absorbing, schedule)


@pytest.mark.parametrize('shape', ['d3_tanh_h48_hopper', 'h50_d2_relu_hopper'])
def test_pwil_worker_with_a_general_actor(shape):
  """The same through il_act_step_general: form (a) appends in k_act_step_general, form (b) in its commit kernel."""
  _worker_matches_separate_calls(shape, 'n600_t40', True, 'exact')


@pytest.mark.parametrize('horizon', [120, 170])
def test_pwil_relabel_memory_matches_the_row_loop(horizon):
  """train.py:135-141: 400 expert rows, ends at rows 99 (terminal), 100 (timeout: two ends in a row), 259 (timeout) and 399 (terminal). Bit-identity with the row loop
  holds for every row. Rows 101 .. 259 and 260 .. 399 are episodes longer than the horizon of 120, so the atoms run out 120 rows into each: from there to the episode's end
  the reference (and with it the oracle, a literal restatement) takes the arg-min of an empty tensor and raises. The kernels - il_pwil_reward and k_pwil_couple alike - end
  such a step when no live atom is left: the reward is reward_scale * exp(-bandwidth * cost) of the cost collected so far (reward_scale itself once nothing is left at the
  step's start), no weight changes. At horizon 120 the oracle comparison therefore covers every row at which the reference defines a reward - 341 of the 400 - at the
  usual bound; the same rows at horizon 170, which no episode outruns, give every row an oracle value."""
  n, D, S = 400, 10, 7
  ends = {99: 'terminals', 100: 'timeouts', 259: 'timeouts', 399: 'terminals'}
  atoms, _ = gi.pwil_case(43, n, D, 1)
  (d_loop, mem_loop), (d_dev, mem_dev) = _discriminator(atoms, S, horizon, ends), _discriminator(atoms, S, horizon, ends)
  untouched = N(mem_dev.ring)
  oracle = opwil.PwilOracle(atoms, horizon, PWIL_CFG['reward_scale'], PWIL_CFG['reward_bandwidth_scale'])

  def loop(first, count):   # the reference's loop, as train.py runs it under +pretraining.schedule=per_function
    want = []
    for i in range(first, first + count):
      tr = mem_loop[i]
      mem_loop.rewards[i] = d_loop.compute_reward(tr['states'].unsqueeze(0), tr['actions'].unsqueeze(0))
      try: want.append(oracle.compute_reward(atoms[i]))
      except ValueError: want.append(np.nan)   # every atom consumed: undefined in the reference until the next reset
      if tr['terminals'] or tr['timeouts']: d_loop.reset(); oracle.reset()
    return np.asarray(want)

  want = loop(0, n)
  d_dev.relabel_memory(mem_dev)
  torch.cuda.synchronize()
  ring, col = N(mem_dev.ring), 2 * S + (D - S)
  np.testing.assert_array_equal(ring[:, col], N(mem_loop.ring)[:, col])
  np.testing.assert_array_equal(N(d_dev.expert_weights), N(d_loop.expert_weights))
  np.testing.assert_array_equal(np.delete(ring, col, axis=1), np.delete(untouched, col, axis=1), err_msg='relabel_memory touched a column other than the rewards')
  defined = ~np.isnan(want)
  if horizon == 120: assert defined[:221].all() and not defined[221:260].any() and defined[260:380].all() and not defined[380:].any()   # 120 rows into each over-long episode
  else: assert defined.all()
  np.testing.assert_allclose(ring[defined, col], want[defined], rtol=2e-5)
  assert (N(d_dev.expert_weights) == np.float32(1 / n)).all(), 'row 399 ends an episode: every atom weight back at 1 / N'

  # a sub-range after a reset(): rows 100 .. 259 (the first one ends an episode at once, the last one too)
  mem_dev.rewards[:] = 0; mem_loop.rewards[:] = 0
  d_dev.reset(); d_loop.reset(); oracle.reset()
  want = loop(100, 160)
  d_dev.relabel_memory(mem_dev, first=100, count=160)
  torch.cuda.synchronize()
  ring = N(mem_dev.ring)
  np.testing.assert_array_equal(ring, N(mem_loop.ring))
  np.testing.assert_array_equal(N(d_dev.expert_weights), N(d_loop.expert_weights))
  defined = ~np.isnan(want)
  assert defined[:121].all() and defined[121:].any() == (horizon != 120) and defined[121:].all() == (horizon != 120)
  np.testing.assert_allclose(ring[100:260, col][defined], want[defined], rtol=2e-5)
  assert (ring[:100, col] == 0).all() and (ring[260:, col] == 0).all()
  d_dev.relabel_memory(mem_dev, first=17, count=0)   # nothing to do is not an error
  with pytest.raises(RuntimeError, match='il_pwil_relabel_rows'):
    _lib.check(_lib.lib().il_pwil_relabel_rows(C.byref(d_dev._desc), _lib.ptr(mem_dev.ring), n, 300, 101, None))


@pytest.mark.parametrize('n,horizon,why', [(3000, 10, 'm > 256'), (6000, 30, 'G m > 4096')], ids=['one_workgroup_size', 'two_launch_size'])
def test_pwil_device_coupling_loud_failures(n, horizon, why):
  """Sizes il_pwil_reward serves with its other kernels: refused by the worker, by relabel_memory and by both entry points, before anything is launched."""
  S, A = gi.DIMS['hopper']
  m, G = int(np.ceil((1 / horizon - 1e-6) * n)) + 2, -(-n // 256)
  assert (m > 256) if why == 'm > 256' else (m <= 256 and G * m > 4096)
  atoms, _ = gi.pwil_case(47, n, S + A, 1)
  disc, mem = _discriminator(atoms, S, horizon)
  before = N(disc.expert_weights), N(mem.ring)
  with pytest.raises(NotImplementedError, match='<= 256.*<= 4096'):
    il.ActingWorker(_actor(S, A, *ACTORS['shipped_h64']), il.ReplayMemory(8, S, A, True, device=DEV), reward_model=disc)
  with pytest.raises(NotImplementedError, match='<= 256.*<= 4096'):
    disc.relabel_memory(mem)
  L = _lib.lib()
  buf = torch.zeros(256, device=DEV)
  unsupported = 2   # IL_ERR_UNSUPPORTED (include/il_hip.h)
  assert L.il_pwil_act_reward(C.byref(disc._desc), _lib.ptr(buf), _lib.ptr(buf), None) == unsupported
  assert b'il_pwil_act_reward' in L.il_last_error() and b'<= 256' in L.il_last_error() and b'<= 4096' in L.il_last_error()
  assert L.il_pwil_relabel_rows(C.byref(disc._desc), _lib.ptr(mem.ring), n, 0, n, None) == unsupported
  assert b'il_pwil_relabel_rows' in L.il_last_error() and b'<= 256' in L.il_last_error() and b'<= 4096' in L.il_last_error()
  assert not L.il_pwil_couple_supported(n, 1 / horizon - 1e-6) and L.il_pwil_couple_supported(25000, 1 / 1000 - 1e-6)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(N(disc.expert_weights), before[0]); np.testing.assert_array_equal(N(mem.ring), before[1])


# ------------------------------------------------------------------------------------------------ train.py
PWIL_RUN = ['algorithm=PWIL', 'env=walker2d']
TRACED_LAUNCHES = 6   # acting launches traced at the start of a run (before training.start: no update launches in between)


def _train(tmp_path, name, extra, monkeypatch, trace=False):
  """One train.py run in its own directory (left again with the test: monkeypatch.chdir). `trace`: the library's launch trace is on over the first acting launches of the
  run and the kernel names it saw are returned."""
  sys.path.insert(0, ROOT)
  import train
  from imitation_learning_amd import config, training as il_training
  seen = {}
  if trace:
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
  il_training._NOISE.clear(); il_training._WS.clear()   # the update noise counter lives with the process: every run starts from zero, like a fresh `python train.py`
  d = tmp_path / name
  d.mkdir()
  monkeypatch.chdir(d)
  score = train.train(config.compose(PWIL_RUN + list(extra) + COMMON))
  if trace: monkeypatch.setattr(il.ActingWorker, '_launch', launch)
  return score, torch.load(d / 'agent.pth', weights_only=False), torch.load(d / 'metrics.pth', weights_only=False), seen


def _same_learner(a, b):
  for part in ('actor', 'critic'):
    assert set(a[part]) == set(b[part])
    for k in a[part]:
      np.testing.assert_array_equal(a[part][k].cpu().numpy(), b[part][k].cpu().numpy(), err_msg=f'{part}: {k}')
  np.testing.assert_array_equal(np.asarray(a['log_alpha'].cpu()), np.asarray(b['log_alpha'].cpu()))


def test_train_py_pwil_default_schedule_trains_the_per_function_learner(tmp_path, monkeypatch):
  """The default schedule (exact: the reference order, the coupling launch in front of each append) against +acting.schedule=per_function: the saved learner bit for bit,
  equal train_returns; and the default run's first acting launches were k_act_step and k_pwil_couple, nothing else (no k_pwil_step, no k_pwil_reset, no copies' kernels)."""
  score_w, agent_w, metrics_w, seen = _train(tmp_path, 'worker', [], monkeypatch, trace=True)
  score_p, agent_p, metrics_p, _ = _train(tmp_path, 'per_function', ['+acting.schedule=per_function'], monkeypatch)
  assert np.isfinite(score_w) and score_w == score_p
  _same_learner(agent_w, agent_p)
  assert len(metrics_w['update_steps']) >= 2 and metrics_w['train_returns'] == metrics_p['train_returns'] and len(metrics_w['train_returns']) >= 2
  for a, b in zip(metrics_w['predicted_rewards'], metrics_p['predicted_rewards']): np.testing.assert_array_equal(a, b)
  assert set(seen) == {'k_act_step', 'k_pwil_couple'} and seen['k_act_step'] == TRACED_LAUNCHES and seen['k_pwil_couple'] == TRACED_LAUNCHES // 2, seen


def test_train_py_pwil_prefill_relabels_the_expert_memory_on_the_device(tmp_path, monkeypatch):
  score_w, agent_w, metrics_w, _ = _train(tmp_path, 'worker', ['imitation.mix_expert_data=prefill_memory'], monkeypatch)
  score_p, agent_p, metrics_p, _ = _train(tmp_path, 'per_function', ['imitation.mix_expert_data=prefill_memory', '+acting.schedule=per_function', '+pretraining.schedule=per_function'], monkeypatch)
  assert np.isfinite(score_w) and score_w == score_p
  _same_learner(agent_w, agent_p)
  assert metrics_w['train_returns'] == metrics_p['train_returns']
  for a, b in zip(metrics_w['predicted_rewards'], metrics_p['predicted_rewards']): np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('schedule', ['fused', 'overlap'])
def test_train_py_pwil_fused_and_overlap_schedules_run(tmp_path, monkeypatch, schedule):
  score, agent, metrics, _ = _train(tmp_path, schedule, [f'+acting.schedule={schedule}'], monkeypatch)
  assert np.isfinite(score)
  assert all(torch.isfinite(v).all() for v in agent['actor'].values()) and all(torch.isfinite(v).all() for v in agent['critic'].values())
  assert len(metrics['update_steps']) >= 2 and all(np.isfinite(q).all() for q in metrics['Q_values']) and all(np.isfinite(e).all() for e in metrics['entropies'])
  assert all(np.isfinite(r).all() and (r >= 0).all() for r in metrics['predicted_rewards'])
