"""`-m gpu`: device-resident expert epochs (`il.PretrainPlan`; il_bc_epoch_steps, il_bc_epoch_steps_general, il_dril_bc_epoch_steps, il_red_epoch_steps).

The expert-data loops of train.py:93-123 - behavioural cloning, the DRIL ensemble, the RED predictor - as ONE library call per table half instead of one gather and
one per-function update per iteration. The plan shares the per-function kernels and reads the same rows in the same order, so everything it leaves behind must equal
the loop's, bit for bit: parameters, Adam moments, step counts, the last loss, and what set_uncertainty_threshold / set_sigma compute afterwards (the models' Philox
call counters advance as the loop's do). Shapes are the smallest that reach every addressing path: a partial last epoch (83 rows: 19 dropped at B = 32), a table of 4
batches that wraps within 7 iterations with both halves refilled, one and two 16-row tiles, a padded tile (B = 24, 20), the tile engine and the layer-at-a-time route of
the general shapes, one and two hidden layers of the DRIL / RED kernels with and without on-chip masks, state_only.
The bodies also run on the host emulation of the kernels (tests/test_pretrain_plan_emulated.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import inputs as gi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib
  from imitation_learning_amd import memory as il_memory
  from gpu_util import DEV, N, T, Cfg, close, close_params

S_, A_, ROWS, K_ = 11, 3, 83, 7   # an absorbing expert memory of 83 rows (state = 10 features + the absorbing flag)


def _expert(rows=ROWS, S=S_, A=A_, absorbing=True, seed=41):
  tr = gi.transitions(np.random.RandomState(seed), rows, S, A, state_shift=0.3, absorbing_frac=0.05 if absorbing else 0.0, weighted=True)
  t = {k: torch.from_numpy(tr[k]) for k in ('states', 'actions', 'rewards', 'next_states', 'terminals', 'timeouts', 'weights')}
  t['num_trajectories'] = 3
  return il.ReplayMemory(rows, S, A, absorbing, transitions=t, device=DEV)


def _actor(H, depth, activation, lr=3e-4, wd=0.01):
  def make():
    torch.manual_seed(7)
    actor = il.SoftActor(S_, A_, Cfg(hidden_size=H, depth=depth, activation=activation), device=DEV)
    actor.flat.copy_(torch.randn(actor.flat.numel(), generator=torch.Generator().manual_seed(11)).to(DEV) * 0.1)
    return actor, il.AdamW(actor, lr=lr, weight_decay=wd)
  return make


def _dril(H, depth, activation, p_in, p):
  def make():
    torch.manual_seed(7)
    m = il.SoftActor(S_, A_, Cfg(hidden_size=H, depth=depth, activation=activation, input_dropout=p_in, dropout=p), device=DEV)
    assert isinstance(m, il.DropoutSoftActor)
    return m, il.AdamW(m, lr=1e-3, weight_decay=0.02)
  return make


def _red(H, depth, activation, p_in, p, state_only=False):
  def make():
    torch.manual_seed(7)
    icfg = Cfg(state_only=state_only, reward_bandwidth_scale=0, discriminator=Cfg(hidden_size=H, depth=depth, activation=activation, input_dropout=p_in, dropout=p))
    m = il.REDDiscriminator(S_, A_, icfg, device=DEV)
    return m, il.AdamW(m, lr=1e-3, weight_decay=0.02)
  return make


# name: (kind, model factory, batch size)
CASES = {
    'bc_fused_b32': ('BC', lambda: _actor(64, 2, 'relu'), 32),                  # two tiles, two batches per epoch, 19 rows dropped: 7 iterations span four epochs
    'bc_fused_b16': ('BC', lambda: _actor(64, 2, 'relu'), 16),                  # a single tile
    'bc_tiles_d3_tanh_h48_b32': ('BC', lambda: _actor(48, 3, 'tanh'), 32),      # general shape, tile engine
    'bc_tiles_d3_tanh_h48_b24': ('BC', lambda: _actor(48, 3, 'tanh'), 24),      # ... with a padded last tile: rows >= n must not read the order table
    'bc_layers_d2_relu_h50_b24': ('BC', lambda: _actor(50, 2, 'relu'), 24),     # general shape outside the tile engine: layer at a time
    'dril_d1_tanh_h64_b32': ('DRIL', lambda: _dril(64, 1, 'tanh', 0.1, 0.2), 32),
    'dril_d2_relu_h32_b20': ('DRIL', lambda: _dril(32, 2, 'relu', 0.4, 0.55), 20),
    'red_d1_relu_h64_b32': ('RED', lambda: _red(64, 1, 'relu', 0.0, 0.0), 32),
    'red_d2_tanh_h64_drop_b20': ('RED', lambda: _red(64, 2, 'tanh', 0.05, 0.4), 20),
    'red_state_only_b32': ('RED', lambda: _red(64, 1, 'relu', 0.05, 0.0, state_only=True), 32),
}


def _loop(kind, model, opt, mem, B, K, seed):
  """train.py::expert_batches + the per-function update: the reference the plan must equal."""
  g, n, count, loss = torch.Generator().manual_seed(seed), mem.size, K, None
  while count > 0:
    order = torch.randperm(n, generator=g).to(torch.int32)
    for lo in range(0, min(n - B + 1, count * B), B):
      batch = il_memory.batch_views(mem.gather(order[lo:lo + B]), mem.state_size, mem.action_size, mem.absorbing)
      loss = il.target_estimation_update(model, batch, opt, want_loss=True) if kind == 'RED' else il.behavioural_cloning_update(model, batch, opt)
      count -= 1
  return loss


def _after(kind, model, mem, B):
  """What train.py:124-128 computes from the pretrained model next: it consumes the model's Philox call counter, which the plan must have left where the loop does."""
  if kind == 'DRIL':
    model.set_uncertainty_threshold(mem['states'][:mem.size], mem['actions'][:mem.size], 0.98)
    return float(model.q)
  if kind == 'RED':
    model.set_sigma(mem['states'][:B], mem['actions'][:B])
    return float(model.sigma_1)
  return 0.0


def _same(a, b, oa, ob, what):
  for name, x, y in (('parameters', a.flat, b.flat), ('exp_avg', oa.exp_avg, ob.exp_avg), ('exp_avg_sq', oa.exp_avg_sq, ob.exp_avg_sq), ('step', oa.step_count[:1], ob.step_count[:1])):
    np.testing.assert_array_equal(N(x), N(y), err_msg=f'{what}: {name}')


@pytest.mark.parametrize('case', list(CASES))
def test_plan_equals_the_per_function_loop_bit_for_bit(case):
  kind, factory, B = CASES[case]
  make, mem = factory(), _expert()
  (ma, oa), (mb, ob) = make(), make()
  before = N(ma.flat)
  plan = il.PretrainPlan(kind, ma, oa, mem, B, torch.Generator().manual_seed(5), chunk_batches=2)   # a table of 4 batches: 7 iterations wrap it and refill both halves
  plan.run(K_)
  want = _loop(kind, mb, ob, mem, B, K_, 5)
  assert not np.array_equal(N(ma.flat), before) and int(N(oa.step_count)[0]) == K_
  _same(ma, mb, oa, ob, case)
  np.testing.assert_array_equal(N(plan.loss).reshape(-1), N(want).reshape(-1), err_msg=f'{case}: last loss')
  assert np.isfinite(N(plan.loss)).all()
  assert int(N(plan.cursor)[0]) == K_
  if kind == 'DRIL': assert ma._act_calls == mb._act_calls == K_
  if kind == 'RED': assert ma._noise_calls == mb._noise_calls == K_
  assert _after(kind, ma, mem, B) == _after(kind, mb, mem, B)
  # ... and a per-function step after the plan sees the state the loop leaves (Adam's device step counter, the models' Philox call counters)
  _loop(kind, ma, oa, mem, B, 1, 9); _loop(kind, mb, ob, mem, B, 1, 9)
  _same(ma, mb, oa, ob, case + ' + one per-function step')


@pytest.mark.parametrize('case', ['bc_fused_b32', 'bc_tiles_d3_tanh_h48_b24', 'bc_layers_d2_relu_h50_b24', 'dril_d2_relu_h32_b20', 'red_d2_tanh_h64_drop_b20'])
def test_split_runs_equal_one_run(case):
  """run(3); run(4) == run(7): the cursor, the noise base and the half-filled table survive a call boundary (3 iterations end in the middle of the second half)."""
  kind, factory, B = CASES[case]
  make, mem = factory(), _expert()
  (ma, oa), (mb, ob) = make(), make()
  pa = il.PretrainPlan(kind, ma, oa, mem, B, torch.Generator().manual_seed(5), chunk_batches=2)
  pa.run(3); pa.run(4)
  pb = il.PretrainPlan(kind, mb, ob, mem, B, torch.Generator().manual_seed(5), chunk_batches=2)
  pb.run(7)
  _same(ma, mb, oa, ob, case)
  np.testing.assert_array_equal(N(pa.loss).reshape(-1), N(pb.loss).reshape(-1))
  assert int(N(pa.cursor)[0]) == int(N(pb.cursor)[0]) == 7
  assert _after(kind, ma, mem, B) == _after(kind, mb, mem, B)


def test_plan_follows_the_reference_record():
  """BASELINE.json configs[0] (tests/golden/bc_config1.npz, the reference's own run): the plan, fed the record's own index table through `orders=`, reaches the reference's
  parameters after 60 iterations within the bound tests/test_reference_backend.py::test_hip_pretraining_follows_the_reference_step_by_step holds the per-function loop to,
  and its last loss is within rtol 2e-5 (+ 2e-5 of the largest loss) of the reference's 60th."""
  from test_reference_backend import A, B, EXPERT_ROWS, S, _reference_record
  K = 60
  g = _reference_record(K)
  z = torch.zeros(EXPERT_ROWS)
  mem = il.ReplayMemory(EXPERT_ROWS, S, A, False, device=DEV, transitions=dict(
      states=torch.from_numpy(g['states']), actions=torch.from_numpy(g['actions']), weights=torch.from_numpy(g['weights']), rewards=z, next_states=torch.from_numpy(g['states']),
      terminals=z, timeouts=z, num_trajectories=1))
  actor = il.SoftActor(S, A, Cfg(hidden_size=256, depth=2, activation='relu'), device=DEV)
  assert actor.flat.numel() == g['init'].size
  actor.flat.copy_(T(g['init']))
  opt = il.AdamW(actor, lr=2.5e-4, weight_decay=0)
  plan = il.PretrainPlan('BC', actor, opt, mem, B, orders=torch.from_numpy(g['idx'].astype(np.int32)), chunk_batches=16)   # 60 iterations: the table of 32 wraps, 4 fills
  plan.run(K)
  last = float(plan.loss)
  print(f'last loss {last:.8e} vs reference {g["losses"][K - 1]:.8e}')
  scale = float(np.abs(g['losses']).max())
  assert abs(last - g['losses'][K - 1]) <= 2e-5 * abs(g['losses'][K - 1]) + 2e-5 * scale, (last, g['losses'][K - 1])
  close_params(N(actor.flat), g['final'], f'actor after {K} plan iterations', 2.5e-4, K, outlier_frac=6e-3)


def test_loud_failures():
  """Fewer expert rows than a batch, a null cursor, steps < 1, n_batches < 1: an error before any launch - nothing is stepped, no counter moves."""
  mem = _expert()
  ma, oa = _actor(64, 2, 'relu')()
  with pytest.raises(RuntimeError, match='at least one full batch'):
    il.PretrainPlan('BC', ma, oa, mem, 96, torch.Generator().manual_seed(0))
  with pytest.raises(ValueError):
    il.PretrainPlan('GAIL', ma, oa, mem, 32, torch.Generator().manual_seed(0))
  with pytest.raises(TypeError):
    il.PretrainPlan('DRIL', ma, oa, mem, 32, torch.Generator().manual_seed(0))
  for case in ('bc_fused_b32', 'bc_tiles_d3_tanh_h48_b32', 'bc_layers_d2_relu_h50_b24', 'dril_d1_tanh_h64_b32', 'red_d1_relu_h64_b32'):
    kind, factory, B = CASES[case]
    m, o = factory()()
    before = N(m.flat)
    plan = il.PretrainPlan(kind, m, o, mem, B, torch.Generator().manual_seed(5), chunk_batches=2)
    cursor = plan.epoch.cursor
    plan.epoch.cursor = None
    with pytest.raises(RuntimeError, match='cursor'): plan.run(1)
    plan.epoch.cursor = cursor
    with pytest.raises(RuntimeError, match='steps'): plan._issue(0)
    with pytest.raises(RuntimeError, match='steps'): plan._issue(-3)
    plan.epoch.n_batches = 0
    with pytest.raises(RuntimeError, match='n_batches'): plan.run(1)
    plan.epoch.n_batches = 4
    gather = plan.ring.gather
    plan.ring.gather = None
    with pytest.raises(RuntimeError, match='order table'): plan.run(1)
    plan.ring.gather = gather
    torch.cuda.synchronize()
    np.testing.assert_array_equal(N(m.flat), before, err_msg=case)
    assert int(N(o.step_count)[0]) == 0 and int(N(plan.cursor)[0]) == 0 and plan.done == 0
    assert getattr(m, '_act_calls', 0) == 0 and getattr(m, '_noise_calls', 0) == 0
    plan.run(2)   # and the plan is still good
    assert int(N(plan.cursor)[0]) == 2 and int(N(o.step_count)[0]) == 2
  # the per-function siblings keep refusing a batch with an order table
  kind, factory, B = CASES['red_d1_relu_h64_b32']
  m, o = factory()()
  plan = il.PretrainPlan(kind, m, o, mem, B, torch.Generator().manual_seed(5), chunk_batches=2)
  rc = _lib.lib().il_red_step(C.byref(plan.desc), C.byref(plan.ring), None, None, None, 1, None, 0, _lib.stream_ptr())
  assert rc != 0 and b'gather' in _lib.lib().il_last_error()


def _train(tmp_path, name, args, settings):
  sys.path.insert(0, ROOT)
  import train
  from imitation_learning_amd import config
  from imitation_learning_amd import training as il_training
  il_training._NOISE.clear(); il_training._WS.clear()   # every run starts from zero, like a fresh `python train.py`
  d = tmp_path / name
  d.mkdir()
  cwd = os.getcwd()
  os.chdir(d)
  try:
    score = train.train(config.compose(args + settings))
  finally:
    os.chdir(cwd)
  out = dict(score=score, agent=torch.load(d / 'agent.pth', weights_only=False))
  if os.path.exists(d / 'discriminator.pth'): out['discriminator'] = torch.load(d / 'discriminator.pth', weights_only=False)
  return out


def _assert_same_checkpoints(a, b):
  assert np.isfinite(a['score']) and a['score'] == b['score']
  for part, sd in a['agent'].items():
    other = b['agent'][part]
    for k, v in (sd.items() if isinstance(sd, dict) else [('', sd)]):
      np.testing.assert_array_equal(v.cpu().numpy(), (other[k] if k else other).cpu().numpy(), err_msg=f'agent.pth {part} {k}')
  assert ('discriminator' in a) == ('discriminator' in b)
  for k, v in a.get('discriminator', {}).items():
    np.testing.assert_array_equal(v.cpu().numpy(), b['discriminator'][k].cpu().numpy(), err_msg=f'discriminator.pth {k}')


def train_both_schedules(tmp_path, args, settings, calls=None):
  plan = _train(tmp_path, 'plan', args, settings)
  n = None if calls is None else len(calls)
  loop = _train(tmp_path, 'per_function', args + ['+pretraining.schedule=per_function'], settings)
  if calls is not None: assert n >= 1 and len(calls) == n, 'the default schedule must go through PretrainPlan, per_function must not'
  _assert_same_checkpoints(plan, loop)
  return plan


@pytest.mark.parametrize('args', [['algorithm=BC', 'env=hopper', 'bc_pretraining.iterations=60'], ['algorithm=RED', 'env=hopper', 'imitation.pretraining.iterations=50']], ids=['BC', 'RED'])
def test_train_py_saves_the_same_checkpoints_under_both_schedules(tmp_path, monkeypatch, args):
  """train.py end to end: the default schedule (PretrainPlan) and `+pretraining.schedule=per_function` write identical agent.pth (and discriminator.pth), bit for bit."""
  from test_train_gpu import COMMON as settings
  calls = []
  real = il.PretrainPlan.run
  monkeypatch.setattr(il.PretrainPlan, 'run', lambda self, n: (calls.append(n), real(self, n))[1])
  out = train_both_schedules(tmp_path, args, settings, calls)
  if args[0] == 'algorithm=RED': assert 'discriminator' in out
