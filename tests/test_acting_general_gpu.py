"""`-m gpu`: the acting worker for GENERAL actor shapes (`il_act_step_general`, csrc/general.hip): any depth 1-8, relu / tanh / sigmoid, wide action spaces.

Form (a) - hidden a multiple of 16 up to 512, state <= 512, 2A <= 16 - is ONE launch (k_act_step_general) and runs under all three schedules; form (b) - every other shape -
is the per-function path's layer-at-a-time launches reading the mailbox plus one commit kernel, under the exact and fused schedules. Either way the worker must do what
`actor(obs).sample()` + `memory.append` + `wrap_for_absorbing_states` do (train.py:151-168): the same actions at the same Philox offsets, bit for bit, and the same ring.
The bodies also run on the host emulation of the kernels (tests/test_acting_general_emulated.py), whose lanes do not run in lockstep."""
import numpy as np
import pytest
import torch

import inputs as gi
from oracle import nets as onets
from oracle import philox
from oracle import replay as oreplay

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib
  from gpu_util import DEV, N, Cfg, close

from test_gpu_parity import _episode_script
from test_timed_path_oracle import record_noise

# name: (dims of tests/golden/inputs.py DIMS, hidden, depth, activation)
FORM_A = {
    'd3_tanh_h48_hopper': ('hopper', 48, 3, 'tanh'),
    'd1_sigmoid_h80_halfcheetah': ('halfcheetah', 80, 1, 'sigmoid'),
    'd2_relu_h320_walker2d': ('walker2d', 320, 2, 'relu'),
    'd8_tanh_h512_ant': ('ant', 512, 8, 'tanh'),
}
FORM_B = {
    'wide_h128_d2': ('wide', 128, 2, 'relu'),       # 2A = 24 > 16
    'h50_d2_relu_hopper': ('hopper', 50, 2, 'relu'),   # hidden not a multiple of 16
}
SHAPES = {**FORM_A, **FORM_B}
CASES = [(s, sch) for s in FORM_A for sch in ('exact', 'fused', 'overlap')] + [(s, sch) for s in FORM_B for sch in ('exact', 'fused')]


def _shape(name):
  env, H, depth, activation = SHAPES[name]
  S, A = gi.DIMS[env]
  return S, A, H, depth, activation


def _actor(S, A, H, depth, activation, seed=3, scale=0.08):
  torch.manual_seed(seed)
  actor = il.SoftActor(S, A, Cfg(hidden_size=H, depth=depth, activation=activation), device=DEV)
  assert actor.general
  actor.flat.copy_(torch.randn_like(actor.flat) * scale)
  return actor


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('shape,schedule', CASES)
def test_general_acting_worker_matches_separate_calls(shape, absorbing, schedule):
  """tests/test_gpu_parity.py::test_acting_worker_matches_separate_calls for general shapes: 60 steps into a ring of 37 rows, both kinds of episode end, a replayed append
  without a new post under overlap. Actions and the whole ring bit-identical to the per-function path, same host cursor / full / trajectory count."""
  S, A, H, depth, activation = _shape(shape)
  actor_a, actor_b = _actor(S, A, H, depth, activation), _actor(S, A, H, depth, activation)
  assert torch.equal(actor_a.flat, actor_b.flat)
  mem_a, mem_b = il.ReplayMemory(37, S, A, absorbing, device=DEV), il.ReplayMemory(37, S, A, absorbing, device=DEV)
  rs = np.random.RandomState(5)
  script = _episode_script(rs, 60, S, absorbing)
  first = rs.standard_normal(S).astype(np.float32); first[-1] = 0.0 if absorbing else first[-1]
  resets = [rs.standard_normal(S).astype(np.float32) * 0.1 for _ in range(8)]
  if absorbing:
    for r in resets: r[-1] = 0.0

  # reference order with the per-function entry points
  acts_a, obs, k = [], torch.from_numpy(first).unsqueeze(0), 0
  for t, (nxt, rew, term, tout) in enumerate(script, 1):
    a = actor_a(obs).sample()
    acts_a.append(N(a))
    nxt_t = torch.from_numpy(nxt).unsqueeze(0)
    mem_a.append(t, obs, a.cpu(), rew, nxt_t, term, tout)
    if term or tout:
      if absorbing and term and not tout: mem_a.wrap_for_absorbing_states()
      obs = torch.from_numpy(resets[k]).unsqueeze(0); k += 1
    else:
      obs = nxt_t

  w = il.ActingWorker(actor_b, mem_b, mirror=schedule == 'overlap')
  assert w.general and w.one_launch == (shape in FORM_A)
  acts_b, k = [], 0
  if schedule == 'exact':
    obs = first
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts_b.append(N(w.act(obs)))
      w.append(t, nxt, rew, term, tout)
      if term or tout: obs = resets[k]; k += 1
      else: obs = nxt
  elif schedule == 'fused':
    a = w.act(first)
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts_b.append(N(a))
      ended = term or tout
      a = w.step(t, nxt, rew, term, tout, obs=resets[k] if ended else None)
      k += int(ended)
  else:  # act on its own stream from the published snapshot (== the live parameters here: nothing updates them), appends on the main stream
    obs, a = first, w.act(first)
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts_b.append(N(a))
      w.post(t, obs, a, nxt, rew, term, tout)
      w.enqueue_append()
      if t % 3 == 0: w.enqueue_append()   # a replayed launch without a new post must append nothing
      ended = term or tout
      obs = resets[k] if ended else nxt
      k += int(ended)
      a = w.act(obs)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(np.concatenate(acts_a), np.concatenate(acts_b))
  np.testing.assert_array_equal(N(mem_a.ring), N(mem_b.ring))
  assert (mem_a.idx, mem_a.full, mem_a.num_trajectories) == (mem_b.idx, mem_b.full, mem_b.num_trajectories)
  assert N(mem_b._ring_state).tolist() == [mem_b.idx, int(mem_b.full), mem_b.size]
  assert mem_a.full, 'the script is meant to wrap the ring'


def _replay_through_the_oracle(S, A, H, depth, activation, schedule, absorbing=True, cap=41, steps=70):
  """The body of tests/test_timed_path_oracle.py::test_acting_launch_replays_through_the_oracle at a general shape: every act's Philox draw recorded (il_noise_fill), the
  oracle's forward (oracle.nets.mlp_forward with the shape's activation) and head on it, ReplayOracle for the ring."""
  torch.manual_seed(17)
  actor = il.SoftActor(S, A, Cfg(hidden_size=H, depth=depth, activation=activation), device=DEV)
  assert actor.general
  rs = np.random.RandomState(8)
  actor.flat.copy_(torch.from_numpy(gi.mlp_params(rs, S, H, depth, 2 * A, out_scale=0.3)).to(DEV))
  mem = il.ReplayMemory(cap, S, A, absorbing, device=DEV)
  omem = oreplay.ReplayOracle(cap, S, A, absorbing)
  layers = onets.unpack(N(actor.flat), onets.mlp_shapes(S, H, depth, 2 * A))
  w = il.ActingWorker(actor, mem)
  key = int(w._seed.value)

  def oracle_action(obs):
    """models.py:90-94 with the draw this act consumed (counter = the actor's act-call count after the launch)."""
    eps = record_noise(key, actor._act_calls & 0xFFFFFFFF, philox.STREAM_ACT, A)
    out, _ = onets.mlp_forward(layers, obs[None, :], activation=activation)
    mean, _, _, std = onets.actor_head(out, A)
    return np.tanh(mean + std * eps[None, :])[0]

  def obs_row():
    o = rs.standard_normal(S).astype(np.float32)
    if absorbing: o[-1] = 0
    return o
  obs = obs_row()
  act = N(w.act(obs))[0]
  close(act, oracle_action(obs), 'first action')
  for t in range(1, steps + 1):
    nxt, rew, term, tout = obs_row(), float(rs.standard_normal()), t in (9, 33, 58), t in (21, 47)
    omem.append(t, obs, act, rew, nxt, term, tout)
    if absorbing and term and not tout:
      omem.wrap_for_absorbing_states()                       # train.py:161
    nobs = obs_row() if (term or tout) else nxt              # env.reset()
    if schedule == 'exact':
      w.append(t, nxt, rew, term, tout)
      a2 = N(w.act(nobs))[0]
    else:
      a2 = N(w.step(t, nxt, rew, term, tout, obs=nobs))[0]
    close(a2, oracle_action(nobs), f'action at step {t}')
    obs, act = nobs, a2
  torch.cuda.synchronize()
  assert (mem.idx, mem.full, mem.num_trajectories) == (omem.idx, omem.full, omem.num_trajectories) and omem.full, 'the script wraps the ring'
  assert N(mem._ring_state).tolist() == [omem.idx, int(omem.full), cap]
  for f in oreplay.FIELDS:
    np.testing.assert_array_equal(N(getattr(mem, f)), getattr(omem, f), err_msg=f)


@pytest.mark.parametrize('schedule', ['exact', 'fused'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_general_acting_replays_through_the_oracle(shape, schedule):
  """il_act_step_general against ReplayOracle + oracle.nets with the recorded Philox draws: the ring bit-exact (the stored action = the returned action), the actions at
  the bound of test_acting_launch_replays_through_the_oracle (gpu_util.close: rtol 1e-5 + 2e-6 of the scale)."""
  _replay_through_the_oracle(*_shape(shape), schedule)


@pytest.mark.parametrize('S,A,H,depth,activation,absorbing', [(300, 4, 64, 2, 'tanh', True), (300, 4, 64, 2, 'tanh', False), (512, 8, 16, 1, 'relu', True)],
                         ids=['row609_absorbing', 'row609_plain', 'row1037_h16'])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_general_acting_rows_wider_than_the_workgroup(S, A, H, depth, activation, absorbing, schedule):
  """A ring row of 2S + A + 5 floats on 256 threads: 609 floats at S = 300 (with and without the absorbing wrap's second row), 1,037 at S = 512 with hidden 16 and A = 8 -
  the shape at which k_gt_fwd's head scratch used to alias its output tile. Against the oracle only: the append loops, the carry copy and the mailbox reads must stride
  over the workgroup, and the cursor must move behind the last barrier (the exact schedule's append-only launches have no other)."""
  _replay_through_the_oracle(S, A, H, depth, activation, schedule, absorbing=absorbing, cap=23, steps=64)


@pytest.mark.parametrize('shape', ['d3_tanh_h48_hopper', 'wide_h128_d2'])
def test_general_acting_greedy(shape):
  S, A, H, depth, activation = _shape(shape)
  actor_a, actor_b = _actor(S, A, H, depth, activation), _actor(S, A, H, depth, activation)
  obs = np.random.RandomState(1).standard_normal(S).astype(np.float32)
  w = il.ActingWorker(actor_b, il.ReplayMemory(8, S, A, True, device=DEV))
  np.testing.assert_array_equal(N(w.act(obs, greedy=True)), N(actor_a.get_greedy_action(torch.from_numpy(obs))))


def test_general_acting_mirror_serves_the_published_parameters():
  """Overlap schedule: the act launch reads the published snapshot, never the live arena. Overwriting actor.flat changes nothing until enqueue_publish."""
  S, A, H, depth, activation = _shape('d3_tanh_h48_hopper')
  actor = _actor(S, A, H, depth, activation)
  old, new = _actor(S, A, H, depth, activation), _actor(S, A, H, depth, activation, seed=4)
  assert torch.equal(old.flat, actor.flat) and not torch.equal(new.flat, actor.flat)
  w = il.ActingWorker(actor, il.ReplayMemory(8, S, A, True, device=DEV), mirror=True)
  obs = np.random.RandomState(2).standard_normal(S).astype(np.float32)
  obs_t = torch.from_numpy(obs).unsqueeze(0)
  actor.flat.copy_(new.flat)   # not published
  torch.cuda.synchronize()
  old._act_calls = actor._act_calls
  np.testing.assert_array_equal(N(w.act(obs)), N(old(obs_t).sample()))
  w.enqueue_publish()
  torch.cuda.synchronize()
  new._act_calls = actor._act_calls
  got = N(w.act(obs))
  np.testing.assert_array_equal(got, N(new(obs_t).sample()))
  old._act_calls = actor._act_calls - 1
  assert not np.array_equal(got, N(old(obs_t).sample())), 'the two parameter sets are meant to act differently'


def test_general_acting_loud_failures():
  L = _lib.lib()
  buf = torch.zeros(4096, device=DEV)
  state = torch.zeros(3, dtype=torch.int64, device=DEV)
  p, ps = _lib.ptr(buf), _lib.ptr(state)
  big = 1 << 30

  def failed(rc):
    return rc != 0 and b'il_act_step_general' in L.il_last_error()
  assert failed(L.il_act_step_general(None, 12, 3, 48, 3, 1, None, None, None, None, 0, 0, None, 0, None, 0, None))
  for missing in range(6):   # each pointer in turn
    args = [p, p, p, p, ps, p]
    args[missing] = None
    assert failed(L.il_act_step_general(args[0], 12, 3, 48, 3, 1, args[1], args[2], args[3], args[4], 0, 0, None, 0, args[5], big, None)), missing
  assert failed(L.il_act_step_general(p, 12, 3, 48, 9, 1, p, p, p, ps, 0, 0, None, 0, p, big, None)) and b'depth' in L.il_last_error()
  assert failed(L.il_act_step_general(p, 12, 3, 48, 3, 3, p, p, p, ps, 0, 0, None, 0, p, big, None)) and b'activation' in L.il_last_error()
  assert failed(L.il_act_step_general(p, 12, 3, 48, 3, 1, p, p, p, ps, 0, 0, None, 0, p, 16, None)) and b'workspace' in L.il_last_error()
  for S, A, H in ((21, 12, 128), (12, 3, 50)):   # form (b): no parameter mirror
    assert failed(L.il_act_step_general(p, S, A, H, 2, 0, p, p, p, ps, 0, 0, ps, 4096, p, big, None)) and b'mirror' in L.il_last_error()
    actor = _actor(S, A, H, 2, 'relu')
    with pytest.raises(NotImplementedError, match='hidden_size a multiple of 16'):
      il.ActingWorker(actor, il.ReplayMemory(8, S, A, True, device=DEV), mirror=True)
    assert not il.ActingWorker(actor, il.ReplayMemory(8, S, A, True, device=DEV)).one_launch
