"""`-m gpu`: populations whose learners differ in state / action width - the four environments of the reference's train_all.py side by side. The `_mixed` entry points
(`il_sac_update_population_mixed`: k_dw_adam_pop_mixed and the tile kernels under the widest learner's LDS allocation; `il_act_step_population_mixed`:
k_act_step_population_mixed; `il_gail_step_population_mixed`: the discriminator launches sized for the widest learner) through `il.BatchedPopulationPlan` and
`il.PopulationActingWorker`. The oracle is this project's own per-learner path through the same arithmetic - `UpdatePlan.run()`, one `il.ActingWorker` per learner,
`il_gail_disc_step` + `il_gail_reward` - so every comparison is bit for bit. Every test that would launch a mixed population first touches a symbol only this feature
adds (`_need_mixed`): without it the test fails on the host, before any launch. The bodies also run on the host emulation of the kernels
(tests/test_mixed_population_emulated.py), which bounds-checks LDS and global accesses: the CPU-side check of the launches' sizing."""
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
  from imitation_learning_amd import training as il_training
  from gpu_util import DEV, N, T, Cfg, fill_memory

import test_population_acting_gpu as tp  # noqa: E402  (episode scripts, the lockstep driver and the per-learner comparison of the uniform population's tests)

W = [(12, 3), (18, 6), (112, 8)]   # hopper, halfcheetah / walker2d and ant with the absorbing bit: the narrowest, a middle and the widest learner
UPDATES = 3


def _need_mixed():
  """The names only this feature adds: an AttributeError here, on the host, instead of a mixed population launched with learner 0's LDS size."""
  L_ = _lib.lib()
  return L_.il_sac_update_population_mixed, L_.il_act_step_population_mixed, L_.il_gail_step_population_mixed


# ---------------------------------------------------------------------------------------------
# 1. SAC update: il.BatchedPopulationPlan over learners of different widths against UpdatePlan.run() per learner
# ---------------------------------------------------------------------------------------------
def _icfg(loss='BCE', H=64):
  return Cfg(state_only=False, spectral_norm=True, loss_function=loss, grad_penalty=1.0, entropy_bonus=0.05, mixup_alpha=1.0, pos_class_prior=0.7, nonnegative_margin=float('inf'),
             discriminator=Cfg(hidden_size=H, depth=1, activation='relu', reward_shaping=False, subtract_log_policy=False, reward_function='AIRL'))


def _plans(widths, B, H=64, algorithm='SAC', loss='BCE', hiddens=None, batches=None):
  """One UpdatePlan per entry of `widths`: own networks, rings, index stream, Philox key and counter (learner_id = position), reproducibly, as
  tests/test_population_gail_mixup_gpu.py::_mixup_plans builds its learners. `hiddens` / `batches`: per-learner overrides for the refusals."""
  il_training._NOISE.clear(); il_training._WS.clear()
  plans, nets_all = [], []
  for l, (S, A) in enumerate(widths):
    torch.manual_seed(40 + l)
    Hl, Bl = (hiddens[l] if hiddens else H), (batches[l] if batches else B)
    cfg = Cfg(hidden_size=Hl, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(40 + l)
    mem = il.ReplayMemory(900, S, A, True, device=DEV); fill_memory(mem, gi.transitions(rs, 400, S, A), 400)
    mem.index_rng = il.IndexStream(100 + l)
    extra, disc = {}, None
    if algorithm != 'SAC':
      emem = il.ReplayMemory(300, S, A, True, device=DEV); fill_memory(emem, gi.transitions(rs, 300, S, A, state_shift=0.5), 300)
      extra = dict(expert_memory=emem)
    if algorithm == 'GAIL':
      icfg = _icfg(loss)
      disc = il.GAILDiscriminator(S, A, icfg, 0.97, device=DEV)
      extra.update(discriminator=disc, discriminator_optimiser=il.AdamW(disc, lr=3e-4, weight_decay=10), imitation_cfg=icfg)
    plans.append(il.UpdatePlan(algorithm, actor, critic, log_alpha, target, mem, ao, co, to, Bl, 0.97, -0.5 * A, 0.99, overlap=False, learner_id=l, **extra))
    nets_all.append((actor, critic, target, log_alpha, ao, co, to, disc, extra.get('discriminator_optimiser')))
  return plans, nets_all


STATE = ('actor', 'critic', 'target', 'log_alpha', 'actor m', 'actor v', 'actor step', 'critic m', 'critic v', 'critic step', 'alpha m', 'alpha v', 'alpha step', 'Philox counter',
         'indices', 'logp', 'q')


def _state(plans, nets_all):
  """Everything an update moves, per learner: the networks, log alpha, all Adam state, the Philox counter, the index draw, logp and q (and, GAIL, the discriminator with its
  optimiser state and buffers, and the rewards)."""
  torch.cuda.synchronize()
  out = []
  for l, ((actor, critic, target, log_alpha, ao, co, to, disc, do), p) in enumerate(zip(nets_all, plans)):
    s = [N(actor.flat), N(critic.flat), N(target.flat), N(log_alpha)]
    for o in (ao, co, to): s += [N(o.exp_avg), N(o.exp_avg_sq), N(o.step_count[:1])]
    s += [N(il_training._NOISE[(p.rows.device, l)]), N(p.idx), N(p.logp), N(p.q)]
    if disc is not None: s += [N(disc.flat), N(disc.sn), N(do.exp_avg), N(do.exp_avg_sq), N(do.step_count[:1]), N(p.rewards), N(p.eidx)]
    out.append(s)
  return out


def _per_learner_updates(widths, B, H, algorithm='SAC', loss='BCE'):
  plans, nets = _plans(widths, B, H, algorithm, loss)
  want = []
  for _ in range(UPDATES):
    for p in plans: p.run()
    want.append(_state(plans, nets))
  return want


def _population_updates(widths, B, H, algorithm='SAC', loss='BCE'):
  plans, nets = _plans(widths, B, H, algorithm, loss)
  pop = il.BatchedPopulationPlan(plans)
  got = []
  for _ in range(UPDATES):
    pop.run()
    got.append(_state(plans, nets))
  return got, pop


def _assert_states_equal(want, got, what):
  for u in range(UPDATES):
    for l, (a_l, b_l) in enumerate(zip(want[u], got[u])):
      assert len(a_l) == len(b_l)
      for i, (a, b) in enumerate(zip(a_l, b_l)):
        assert np.isfinite(a.astype(np.float64)).all(), (u, l, i)
        np.testing.assert_array_equal(a, b, err_msg=f'{what}: update {u}, learner {l}: {STATE[i] if i < len(STATE) else f"discriminator tensor {i - len(STATE)}"}')


ORDERS = {'narrowest-first': W, 'widest-first': W[::-1], 'nine-learners': [W[l % 3] for l in range(9)]}


@pytest.mark.parametrize('order', list(ORDERS))
@pytest.mark.parametrize('B,H', [(64, 64), (48, 64), (64, 128)], ids=['B64-H64-blocks', 'B48-H64-tiles', 'B64-H128-blocks'])
def test_mixed_sac_population_equals_plan_run_per_learner(B, H, order):
  """Three updates of learners of widths W through BatchedPopulationPlan (il_sac_update_population_mixed) against UpdatePlan.run() per learner: actor, critic, target,
  log alpha, all Adam state, the Philox counter, the index draw, logp and q bit for bit after every update. B = 64: the optimiser launches' 64 x 64 block path with the
  fused target step (a narrower learner's surplus workgroups must end before they reach the tail; the actor launch's tail must get the learner's own index and count);
  B = 48: the wave-per-tile path, three tiles. Narrowest learner first (the launch's shape descriptor is the narrowest), widest first, and nine learners cycling through
  W: more than the 8 XCDs, so the first eight learners' workgroups are re-labelled and the ninth keeps the natural decode."""
  _need_mixed()
  widths = ORDERS[order]
  want = _per_learner_updates(widths, B, H)
  got, pop = _population_updates(widths, B, H)
  assert pop.mixed and pop.algorithm == 'SAC' and pop.L == len(widths)
  _assert_states_equal(want, got, f'B={B} H={H} {order}')
  assert not np.array_equal(got[0][0][0], got[UPDATES - 1][0][0]) and not np.array_equal(got[0][0][2], got[UPDATES - 1][0][2]), 'the updates are meant to move the actor and the target'
  assert all(int(got[u][l][13][0]) == u + 1 for u in range(UPDATES) for l in range(len(widths))), 'one counter bump per learner and update'
  assert all(int(got[UPDATES - 1][l][k][0]) == UPDATES for l in range(len(widths)) for k in (6, 9, 12)), 'one optimiser step per learner, network and update'


@pytest.mark.parametrize('B', [64, 48])
def test_uniform_population_of_each_width_gives_the_mixed_population_s_bytes(B):
  """Learner l of the mixed population against learner 0 of a UNIFORM population (il_sac_update_population, unchanged) of three learners of width W[l] built under the same
  seeds and learner id: the uniform launch keeps its grids and its bits, and the mixed one adds nothing to them."""
  _need_mixed()
  got, _ = _population_updates(W, B, 64)
  for l, w in enumerate(W):
    # position l of the uniform population is built like position l of the mixed one (same seeds, same learner_id); the other positions are its neighbours
    uni, pop = _population_updates([w, w, w], B, 64)
    assert not pop.mixed
    for u in range(UPDATES):
      for i, (a, b) in enumerate(zip(got[u][l], uni[u][l])):
        np.testing.assert_array_equal(a, b, err_msg=f'B={B}: update {u}, width {w}: {STATE[i]}')


# ---------------------------------------------------------------------------------------------
# 2. Acting: il.PopulationActingWorker over learners of different widths against one il.ActingWorker per learner
# ---------------------------------------------------------------------------------------------
def _mixed_actors_and_memories(widths, H, absorbing, capacity=tp.CAPACITY):
  """tests/test_population_acting_gpu.py::_actors_and_memories with a width per learner: two identical sets."""
  cfg = Cfg(hidden_size=H, depth=2, activation='relu')
  sets, mems = ([], []), ([], [])
  for l, (S, A) in enumerate(widths):
    torch.manual_seed(11 + l)
    flat = None
    for side, ms in zip(sets, mems):
      actor = il.SoftActor(S, A, cfg, device=DEV)
      if flat is None: flat = torch.randn_like(actor.flat) * 0.08
      actor.flat.copy_(flat)
      side.append(actor)
      ms.append(il.ReplayMemory(capacity, S, A, absorbing, device=DEV))
  return sets[0], sets[1], mems[0], mems[1]


def _pop_actions(run, widths):
  """The lockstep driver keeps [1, widest A] rows per learner: learner l's own components, and zeros behind them."""
  out = []
  for l, (_, A) in enumerate(widths):
    a = np.stack([x.reshape(-1) for x in run.acts[l]])
    assert (a[:, A:] == 0).all(), f'learner {l}: components behind its own {A} are meant to be zero'
    out.append(a[:, :A])   # [steps, A_l], as _run_single leaves the single worker's
  return out


@pytest.mark.parametrize('absorbing', [True, False])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
@pytest.mark.parametrize('H', [64, 128])
def test_mixed_population_acting_matches_per_learner_workers(H, schedule, absorbing):
  """60 lockstep steps of three learners of widths W into rings of 37 rows, each with its own episode script, actor parameters and Philox seed (the scripts of the uniform
  population's test): actions, whole rings, device cursors, host mirrors and `_act_calls` are those of one ActingWorker per learner. Learner 2's row has 237 floats."""
  _need_mixed()
  L = len(W)
  actors_a, actors_b, mems_a, mems_b = _mixed_actors_and_memories(W, H, absorbing)
  scripts = [tp._learner_script(l, tp.STEPS, W[l][0], absorbing, last_row=l == 1) for l in range(L)]
  seeds = [1000 + 17 * l for l in range(L)]
  acts_ref = [tp._run_single(il.ActingWorker(actors_a[l], mems_a[l], noise_seed=seeds[l]), schedule, *scripts[l]) for l in range(L)]
  w = il.PopulationActingWorker(actors_b, mems_b, seeds)
  assert w.mixed and w.widths == W
  run = tp._Lockstep(w, schedule, scripts)
  for _ in range(tp.STEPS):
    run.launch(list(range(L)))
  torch.cuda.synchronize()
  tp._assert_learners_equal(acts_ref, _pop_actions(run, W), actors_a, actors_b, mems_a, mems_b)
  assert all(m.full for m in mems_b), 'the scripts are meant to wrap every ring'


@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_mixed_population_acting_idle_learner(schedule):
  """Learner 1 idles for launches 15..24 while the narrower and the wider learner act, and the launches of steps 5, 20 and 30 are issued twice without a new post."""
  _need_mixed()
  L, absorbing = len(W), True
  actors_a, actors_b, mems_a, mems_b = _mixed_actors_and_memories(W, 64, absorbing)
  lengths = [50 if l != 1 else 40 for l in range(L)]
  scripts = [tp._learner_script(l, lengths[l], W[l][0], absorbing) for l in range(L)]
  seeds = [77 + l for l in range(L)]
  acts_ref = [tp._run_single(il.ActingWorker(actors_a[l], mems_a[l], noise_seed=seeds[l]), schedule, *scripts[l]) for l in range(L)]
  w = il.PopulationActingWorker(actors_b, mems_b, seeds)
  run = tp._Lockstep(w, schedule, scripts)
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
  tp._assert_learners_equal(acts_ref, _pop_actions(run, W), actors_a, actors_b, mems_a, mems_b)


def test_mixed_evaluate_population_equals_evaluate_agent():
  """Three synthetic environments of different widths (hopper, halfcheetah, ant) and horizons: evaluate_population over the mixed worker returns evaluate_agent's lists
  and leaves every `_act_calls` where evaluate_agent leaves it."""
  _need_mixed()
  from imitation_learning_amd.environments import SyntheticD4RLEnv
  from imitation_learning_amd.evaluation import evaluate_agent, evaluate_population
  names, horizons, absorbing, episodes = ('hopper', 'halfcheetah', 'ant'), (20, 35, 50), True, 2
  envs_a = [SyntheticD4RLEnv(n, absorbing, max_episode_steps=h) for n, h in zip(names, horizons)]
  envs_b = [SyntheticD4RLEnv(n, absorbing, max_episode_steps=h) for n, h in zip(names, horizons)]
  for l, (ea, eb) in enumerate(zip(envs_a, envs_b)):
    ea.seed(40 + l); eb.seed(40 + l)
  widths = [(e.observation_space.shape[0], e.action_space.shape[0]) for e in envs_a]
  assert widths == W
  actors_a, actors_b, mems_a, mems_b = _mixed_actors_and_memories(widths, 64, absorbing)
  want = [evaluate_agent(actors_a[l], envs_a[l], episodes) for l in range(3)]
  w = il.PopulationActingWorker(actors_b, mems_b, [5, 6, 7])
  got = evaluate_population(w, envs_b, episodes)
  torch.cuda.synchronize()
  assert got == want and all(len(g) == episodes for g in got)
  assert [a._act_calls for a in actors_a] == [b._act_calls for b in actors_b]


# ---------------------------------------------------------------------------------------------
# 3. GAIL: il_gail_step_population_mixed against il_gail_disc_step + il_gail_reward per learner
# ---------------------------------------------------------------------------------------------
class _Learner:
  pass


def _disc_learners(widths, B, loss, seed=3):
  """One discriminator per width with everything it owns (tests/test_population_gail_mixup_gpu.py::_learners, a width per learner)."""
  out = []
  for l, (S, A) in enumerate(widths):
    ln = _Learner()
    torch.manual_seed(1000 * seed + l)
    rs = np.random.RandomState(1000 * seed + l)
    ln.icfg = _icfg(loss)
    ln.disc = il.GAILDiscriminator(S, A, ln.icfg, 0.97, device=DEV)
    ln.opt = il.AdamW(ln.disc, lr=3e-4, weight_decay=10.0)
    n = ln.opt.exp_avg.numel()
    ln.opt.exp_avg.copy_(T((1e-3 * rs.standard_normal(n)).astype(np.float32))); ln.opt.exp_avg_sq.copy_(T((1e-6 * rs.uniform(0.5, 1.5, n)).astype(np.float32)))
    ln.opt.step_count[0] = 2 + l
    ln.d = il_training.disc_descriptor(ln.disc, B, ln.opt, ln.icfg, tag=('mixed-population', seed, l))
    ln.ctr = torch.tensor([5 + 3 * l], dtype=torch.int32, device=DEV)
    ln.d.noise_seed, ln.d.noise_counter = 90001 + 7919 * l, ln.ctr.data_ptr()
    ln.pol = {k: T(v) for k, v in gi.transitions(rs, B, S, A, weighted=True).items()}
    ln.exp = {k: T(v) for k, v in gi.transitions(rs, B, S, A, state_shift=0.5, weighted=True).items()}
    ln.pb, ln.eb = il_memory.batch_desc(ln.pol), il_memory.batch_desc(ln.exp)
    ln.rewards = torch.full((B,), -7.5, device=DEV)
    out.append(ln)
  return out


def _disc_snapshot(learners):
  torch.cuda.synchronize()
  return [[N(ln.disc.flat), N(ln.opt.exp_avg), N(ln.opt.exp_avg_sq), N(ln.opt.step_count[:1]), N(ln.opt.grad), N(ln.rewards), N(ln.disc.sn)] for ln in learners]


def _mixed_gail_args(learners):
  descs = il_training._device_array([ln.d for ln in learners], DEV)
  pol, exp = il_training._device_array([ln.pb for ln in learners], DEV), il_training._device_array([ln.eb for ln in learners], DEV)
  rewards = torch.tensor([ln.rewards.data_ptr() for ln in learners], dtype=torch.int64, device=DEV)
  host = (_lib.Disc * len(learners))(*[ln.d for ln in learners])
  return [_lib.ptr(descs), _lib.ptr(pol), _lib.ptr(exp), _lib.ptr(rewards), len(learners), C.cast(host, C.c_void_p)], (descs, pol, exp, rewards, host)


@pytest.mark.parametrize('widths', [W, W[::-1]], ids=['narrowest-first', 'widest-first'])
@pytest.mark.parametrize('loss', ['BCE', 'PUGAIL'])
def test_mixed_gail_step_population_equals_the_per_learner_sequence(loss, widths):
  """il_gail_step_population_mixed over discriminators (hidden 64) of widths W at B = 64, BCE and PUGAIL with an infinite margin, three updates with every learner's
  update counter bumped in between: parameters, m, v, step, gradient arena, rewards and the u / v buffers equal il_gail_disc_step + il_gail_reward per learner."""
  fn = _need_mixed()[2]
  L_, st, B = _lib.lib(), _lib.stream_ptr(), 64
  ref = _disc_learners(widths, B, loss)
  want = []
  for _ in range(UPDATES):
    for ln in ref:
      _lib.check(L_.il_gail_disc_step(C.byref(ln.d), C.byref(ln.pb), C.byref(ln.eb), None, None, 0, st))
      _lib.check(L_.il_gail_reward(C.byref(ln.d), C.byref(ln.pb), _lib.ptr(ln.rewards), None, None, st))
    want.append(_disc_snapshot(ref))
    for ln in ref: ln.ctr.add_(1)
  learners = _disc_learners(widths, B, loss)
  args, keep = _mixed_gail_args(learners)
  for u in range(UPDATES):
    _lib.check(fn(*args, st))
    got = _disc_snapshot(learners)
    for l in range(len(widths)):
      for name, a, b in zip(('parameters', 'm', 'v', 'step', 'gradient arena', 'rewards', 'u / v buffers'), want[u][l], got[l]):
        assert np.isfinite(a.astype(np.float64)).all(), (u, l, name)
        np.testing.assert_array_equal(a, b, err_msg=f'{loss}: update {u}, learner {l} (widths {widths[l]}): {name}')
    for ln in learners: ln.ctr.add_(1)
  assert not np.array_equal(want[0][0][0], want[UPDATES - 1][0][0]), 'the updates are meant to move the parameters'


@pytest.mark.parametrize('loss', ['BCE', 'PUGAIL'])
def test_mixed_gail_population_plan_equals_plan_run_per_learner(loss):
  """BatchedPopulationPlan of GAIL learners of widths W (the discriminator launches on the side stream beside the forward kernels) against plan.run() per learner."""
  _need_mixed()
  want = _per_learner_updates(W, 64, 64, 'GAIL', loss)
  got, pop = _population_updates(W, 64, 64, 'GAIL', loss)
  assert pop.mixed and pop.algorithm == 'GAIL' and pop._disc_host is not None
  _assert_states_equal(want, got, f'GAIL {loss}')


# ---------------------------------------------------------------------------------------------
# 4. Loud failures, all on the host, before any launch
# ---------------------------------------------------------------------------------------------
def test_mixed_population_plan_refusals():
  _need_mixed()
  with pytest.raises(AssertionError, match='one hidden size'):
    il.BatchedPopulationPlan(_plans(W, 64, hiddens=[64, 128, 64])[0])
  with pytest.raises(AssertionError, match='one batch size'):
    il.BatchedPopulationPlan(_plans(W, 64, batches=[64, 48, 64])[0])
  with pytest.raises(AssertionError, match='Mixup'):
    il.BatchedPopulationPlan(_plans(W, 64, algorithm='GAIL', loss='Mixup')[0])


def _red_plans(widths):
  il_training._NOISE.clear(); il_training._WS.clear()
  plans = []
  for l, (S, A) in enumerate(widths):
    torch.manual_seed(40 + l)
    cfg = Cfg(hidden_size=64, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(40 + l)
    mem = il.ReplayMemory(300, S, A, True, device=DEV); fill_memory(mem, gi.transitions(rs, 200, S, A), 200)
    emem = il.ReplayMemory(300, S, A, True, device=DEV); fill_memory(emem, gi.transitions(rs, 200, S, A, state_shift=0.5), 200)
    red = il.REDDiscriminator(S, A, Cfg(state_only=False, reward_bandwidth_scale=None, discriminator=Cfg(hidden_size=32, depth=1, activation='relu', input_dropout=0, dropout=0)), device=DEV)
    red.sigma_1 = 0.5
    red.eval()
    plans.append(il.UpdatePlan('RED', actor, critic, log_alpha, target, mem, ao, co, to, 64, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=red,
                               discriminator_optimiser=il.AdamW(red, lr=3e-5, weight_decay=0), overlap=False, learner_id=l))
  return plans


def _dril_plans(widths):
  """DRIL learners (tests/test_population_dril_gpu.py::_dril_learners) with a width per learner: the shipped ensemble shape, each with its threshold set."""
  il_training._NOISE.clear(); il_training._WS.clear()
  plans = []
  mcfg = Cfg(hidden_size=64, depth=1, activation='tanh', input_dropout=0.1, dropout=0.1)
  for l, (S, A) in enumerate(widths):
    torch.manual_seed(40 + l)
    cfg = Cfg(hidden_size=64, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(40 + l)
    agent, expert = gi.transitions(rs, 200, S, A), gi.transitions(rs, 200, S, A, state_shift=0.5)
    agent['actions'], expert['actions'] = (0.8 * agent['actions']).astype(np.float32), (0.8 * expert['actions']).astype(np.float32)
    mem = il.ReplayMemory(300, S, A, True, device=DEV); fill_memory(mem, agent, 200)
    emem = il.ReplayMemory(300, S, A, True, device=DEV); fill_memory(emem, expert, 200)
    disc = il.DropoutSoftActor(S, A, mcfg, device=DEV)
    disc.flat.mul_(0.3)
    disc.q = 0.5   # (a threshold of any value: the plan only asks that one is set; no launch is meant to happen here)
    plans.append(il.UpdatePlan('DRIL', actor, critic, log_alpha, target, mem, ao, co, to, 64, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=disc,
                               discriminator_optimiser=il.AdamW(disc, lr=3e-5, weight_decay=0), overlap=False, learner_id=l, bc_aux=True))
  return plans


def test_mixed_widths_with_other_algorithms_are_refused():
  """RED and DRIL keep their `share dims` assertions; an algorithm whose step has no width check of its own (PWIL: SAC's update, the rewards stored while acting) is refused by the
  plan's mixed-width check, which names SAC and GAIL."""
  _need_mixed()
  with pytest.raises(AssertionError, match='share dims'):
    il.BatchedPopulationPlan(_red_plans(W))
  with pytest.raises(AssertionError, match='share dims'):
    il.BatchedPopulationPlan(_dril_plans(W))
  plans = _plans(W, 64)[0]
  for p in plans: p.algorithm = 'PWIL'   # (a PWIL plan is a SAC plan whose rewards were stored by the acting side: only the name differs here)
  with pytest.raises(AssertionError, match='SAC and GAIL only'):
    il.BatchedPopulationPlan(plans)


def test_mixed_acting_worker_refusals():
  _need_mixed()
  actors, _, mems, _ = _mixed_actors_and_memories(W, 64, True)
  other = il.SoftActor(18, 6, Cfg(hidden_size=128, depth=2, activation='relu'), device=DEV)
  with pytest.raises(AssertionError, match='one hidden size'):
    il.PopulationActingWorker([actors[0], other, actors[2]], mems, [1, 2, 3])
  with pytest.raises(AssertionError, match='feeds a memory'):
    il.PopulationActingWorker([actors[1], actors[0], actors[2]], mems, [1, 2, 3])
  # a learner whose own widths break il_act_step's limits: at hidden 64 the workgroup has 256 threads, and 64 + 200 state floats do not fit
  wide = [(12, 3), (200, 4)]
  a2, _, m2, _ = _mixed_actors_and_memories(wide, 64, True)
  with pytest.raises(AssertionError, match="learner 1 .* outside il_act_step's limits"):
    il.PopulationActingWorker(a2, m2, [1, 2])

  class Reward:
    pass
  with pytest.raises(NotImplementedError, match='one shape for all learners|PWIL'):
    il.PopulationActingWorker(actors, mems, [1, 2, 3], reward_models=[Reward(), Reward(), Reward()])


def test_mixed_entry_points_refuse_bad_arguments():
  """Null or zero-learner arguments, and learners outside the limits, to each new entry point: a nonzero return and an il_last_error text that names the entry point."""
  sac, act, gail = _need_mixed()
  L_ = _lib.lib()
  some = torch.zeros(256, dtype=torch.float32, device=DEV)
  p = _lib.ptr(some)

  def refused(fn, name, args, word):
    assert fn(*args) != 0, (name, word)
    err = L_.il_last_error()
    assert name in err and word in err, (name, word, err)

  host = (_lib.Sac * 2)()
  for d, (S, A) in zip(host, [(12, 3), (18, 6)]): d.state_dim, d.action_dim, d.hidden, d.batch = S, A, 64, 64
  hp = C.cast(host, C.c_void_p)
  refused(sac, b'il_sac_update_population_mixed', (None, p, 2, hp, 0, None), b'null')
  refused(sac, b'il_sac_update_population_mixed', (p, None, 2, hp, 0, None), b'null')
  refused(sac, b'il_sac_update_population_mixed', (p, p, 2, None, 0, None), b'null')
  refused(sac, b'il_sac_update_population_mixed', (p, p, 0, hp, 0, None), b'n_learners=0')
  refused(sac, b'il_sac_update_population_mixed', (p, p, 2, hp, _lib.IL_FLAG_GRADS_ONLY, None), b'IL_FLAG_GRADS_ONLY')
  refused(sac, b'il_sac_update_population_mixed', (p, p, 2, hp, 0, None), b'learner 0: workspace too small')
  host[1].hidden = 128
  refused(sac, b'il_sac_update_population_mixed', (p, p, 2, hp, 0, None), b'learner 1 has hidden=128')
  host[1].hidden, host[1].batch = 64, 48
  refused(sac, b'il_sac_update_population_mixed', (p, p, 2, hp, 0, None), b'learner 1 has batch=48')
  host[1].batch, host[1].action_dim = 64, 9
  refused(sac, b'il_sac_update_population_mixed', (p, p, 2, hp, 0, None), b'learner 1: action_dim=9')

  row = lambda S, A: int(L_.il_ring_row_floats(S, A))
  dims = (_lib.ActDims * 2)(_lib.ActDims(12, 3, row(12, 3), 0), _lib.ActDims(18, 6, row(18, 6), 0))
  dp = C.cast(dims, C.c_void_p)
  refused(act, b'il_act_step_population_mixed', (None, p, dp, 2, 64, None), b'null')
  refused(act, b'il_act_step_population_mixed', (p, None, dp, 2, 64, None), b'null')
  refused(act, b'il_act_step_population_mixed', (p, p, None, 2, 64, None), b'null')
  refused(act, b'il_act_step_population_mixed', (p, p, dp, 0, 64, None), b'no learner')
  refused(act, b'il_act_step_population_mixed', (p, p, dp, 2, 96, None), b'hidden=96')
  dims[1].ring_row_floats += 4
  refused(act, b'il_act_step_population_mixed', (p, p, dp, 2, 64, None), b'learner 1: ring_row_floats')
  dims[1] = _lib.ActDims(200, 4, row(200, 4), 0)
  refused(act, b'il_act_step_population_mixed', (p, p, dp, 2, 64, None), b'learner 1: ring row')
  dims[1] = _lib.ActDims(18, 9, row(18, 9), 0)
  refused(act, b'il_act_step_population_mixed', (p, p, dp, 2, 64, None), b'learner 1: unsupported dims')

  learners = _disc_learners([(12, 3), (18, 6)], 64, 'BCE')
  before = _disc_snapshot(learners)
  args, keep = _mixed_gail_args(learners)
  for i in (0, 1, 2, 3, 5):
    a = list(args); a[i] = None
    refused(gail, b'il_gail_step_population_mixed', (*a, None), b'null')
  a = list(args); a[4] = 0
  refused(gail, b'il_gail_step_population_mixed', (*a, None), b'n_learners=0')
  host = keep[4]
  host[1].hidden = 128
  refused(gail, b'il_gail_step_population_mixed', (*args, None), b'learner 1 has hidden=128')
  host[1].hidden, host[1].spectral_norm = 64, 0
  refused(gail, b'il_gail_step_population_mixed', (*args, None), b'learner 1 differs')
  host[1].spectral_norm = 1
  host[0].loss_function = 2
  refused(gail, b'il_gail_step_population_mixed', (*args, None), b'Mixup')
  host[0].loss_function, host[0].pu_clamped = 1, 1
  refused(gail, b'il_gail_step_population_mixed', (*args, None), b'pu_clamped')
  for a_l, b_l in zip(before, _disc_snapshot(learners)):
    for x, y in zip(a_l, b_l): np.testing.assert_array_equal(x, y, err_msg='a refused call launched a kernel')


def test_replay_sample_population_serves_rows_of_different_widths():
  """il_replay_sample_population already carries row_floats per learner (and the launch's max_row_floats): the index draws and gathered rows of the mixed population's
  first update are those of every learner's own plan - confirmed here, the entry point is unchanged."""
  _need_mixed()
  plans, nets = _plans(W, 64)
  for p in plans: p.run()
  torch.cuda.synchronize()
  want = [(N(p.idx), N(p.rows)) for p in plans]
  plans, nets = _plans(W, 64)
  pop = il.BatchedPopulationPlan(plans)
  assert pop.max_row == max(p.memory.row for p in plans) and len({p.memory.row for p in plans}) == 3
  pop.run()
  torch.cuda.synchronize()
  for l, p in enumerate(plans):
    np.testing.assert_array_equal(want[l][0], N(p.idx), err_msg=f'learner {l}: indices')
    np.testing.assert_array_equal(want[l][1], N(p.rows), err_msg=f'learner {l}: rows')


# ---------------------------------------------------------------------------------------------
# 5. train_all.py: the four environments as one population, population schedule against per_learner
# ---------------------------------------------------------------------------------------------
from test_train_gpu import COMMON  # noqa: E402  (steps 260, batch 64, two evaluations of two episodes, 60-step episodes)

ENVS = ['ant', 'halfcheetah', 'hopper', 'walker2d']


def _train_all(tmp_path, name, argv, multirun=False):
  """One `python train_all.py ...` in this process, from a fresh working directory and fresh process-wide update counters."""
  if ROOT not in sys.path: sys.path.insert(0, ROOT)
  import train_all   # (a name only this feature adds: ImportError on the host without it)
  _need_mixed()
  il_training._NOISE.clear(); il_training._WS.clear()
  d = tmp_path / name
  d.mkdir()
  before = os.getcwd()
  os.chdir(d)
  try:
    return (train_all.multirun if multirun else train_all.train_all)(argv, stamp=name)
  finally:
    os.chdir(before)


def _env_files(root):
  return {env: {f: torch.load(os.path.join(root, env, f), weights_only=False) for f in sorted(os.listdir(os.path.join(root, env))) if f.endswith('.pth')} for env in sorted(os.listdir(root))}


def _assert_same_runs(fa, fb, what, files):
  assert sorted(fa) == sorted(fb) == ENVS, what
  for env in ENVS:
    assert set(fa[env]) == set(fb[env]) == files, (what, env)
    for f in files:
      a, b = ({k: v for k, v in m.items() if k not in tp.TIMING_KEYS} for m in (fa[env][f], fb[env][f]))
      tp._assert_same_nested(a, b, f'{what}: {env}/{f}')


def train_all_schedules_leave_the_same_bytes(tmp_path, algorithm, short, min_updates=2):
  """`train_all.py algorithm=<ALG> seed=3` under +sweep.schedule=population and per_learner: the same four directories, files and bytes (timing keys aside); finite scores
  whose minimum is the return value; four different actors."""
  files = {'agent.pth', 'metrics.pth'} | ({'discriminator.pth'} if algorithm == 'GAIL' else set())
  argv = [f'algorithm={algorithm}', 'seed=3'] + short
  root_p, scores_p, worst_p = _train_all(tmp_path, 'population', argv + ['+sweep.schedule=population'])
  root_l, scores_l, worst_l = _train_all(tmp_path, 'per_learner', argv + ['+sweep.schedule=per_learner'])
  assert os.path.basename(os.path.dirname(root_p)) == f'{algorithm}_all' and sorted(os.listdir(root_p)) == ENVS == sorted(os.listdir(root_l))
  assert sorted(scores_p) == ENVS and np.isfinite(list(scores_p.values())).all() and scores_p == scores_l
  assert worst_p == min(scores_p.values()) == worst_l
  fp, fl = _env_files(root_p), _env_files(root_l)
  _assert_same_runs(fp, fl, f'{algorithm}: population against per_learner', files)
  for env in ENVS:
    m = fp[env]['metrics.pth']
    assert len(m['update_steps']) >= min_updates and len(m['test_steps']) == 2 and all(np.isfinite(q).all() for q in m['Q_values'])
    assert all(torch.isfinite(v).all() for v in fp[env]['agent.pth']['actor'].values())
  shapes = {env: tuple(fp[env]['agent.pth']['actor'][k].shape for k in sorted(fp[env]['agent.pth']['actor'])) for env in ENVS}
  assert len(set(shapes.values())) == 3, 'ant, hopper and the halfcheetah / walker2d pair have actors of three shapes'
  a, b = fp['halfcheetah']['agent.pth']['actor'], fp['walker2d']['agent.pth']['actor']
  assert any(not torch.equal(v, b[k]) for k, v in a.items()), 'the two learners of one shape are meant to differ'
  return root_p, fp


@pytest.mark.parametrize('algorithm', ['SAC', 'GAIL'])
def test_train_all_population_equals_per_learner(tmp_path, algorithm):
  train_all_schedules_leave_the_same_bytes(tmp_path, algorithm, COMMON)


def test_train_all_graph_replays_equal_direct_launches(tmp_path, monkeypatch, short=None):
  """IL_TRAIN_LAUNCH=graph captures the mixed population's update after its first, eager, run and replays it: the direct launches' bytes."""
  argv = ['algorithm=GAIL', 'seed=3', '+sweep.schedule=population'] + (short or COMMON)
  monkeypatch.setenv('IL_TRAIN_LAUNCH', 'direct')
  root_d, scores_d, _ = _train_all(tmp_path, 'direct', argv)
  monkeypatch.setenv('IL_TRAIN_LAUNCH', 'graph')
  root_g, scores_g, _ = _train_all(tmp_path, 'graph', argv)
  assert np.isfinite(list(scores_d.values())).all() and scores_d == scores_g
  _assert_same_runs(_env_files(root_d), _env_files(root_g), 'graph replays against direct launches', {'agent.pth', 'discriminator.pth', 'metrics.pth'})


def test_train_all_multirun_of_two_seeds_is_one_population_of_eight(tmp_path, capsys, short=None):
  """`train_all.py -m seed=3,4 algorithm=SAC +sweep.schedule=population`: ONE population of eight learners; job j's bytes are those of `train_all.py seed=<its seed>` alone
  under the same schedule."""
  short = short or COMMON
  capsys.readouterr()
  root, scores, worst = _train_all(tmp_path, 'sweep', ['-m', 'seed=3,4', 'algorithm=SAC', '+sweep.schedule=population'] + short, multirun=True)
  err = capsys.readouterr().err
  assert err.count('[train_all]') == 1 and '8 learners' in err and 'train as one population' in err, err
  assert os.path.basename(os.path.dirname(root)) == 'SAC_all_sweeper' and sorted(os.listdir(root)) == ['0', '1']
  assert worst == [min(s.values()) for s in scores] and np.isfinite(worst).all()
  for j, seed in enumerate((3, 4)):
    alone, scores_alone, worst_alone = _train_all(tmp_path, f'alone{seed}', ['algorithm=SAC', f'seed={seed}', '+sweep.schedule=population'] + short)
    _assert_same_runs(_env_files(os.path.join(root, str(j))), _env_files(alone), f'job {j} against seed {seed} alone', {'agent.pth', 'metrics.pth'})
    assert scores[j] == scores_alone and worst[j] == worst_alone


def test_train_all_without_mixed_population_launches_trains_environment_after_environment(tmp_path, capsys, short=None):
  """PWIL has no population launches for learners of different widths: the four environments run one after another through train(), the reason goes to stderr, and the
  four directories are complete."""
  capsys.readouterr()
  root, scores, worst = _train_all(tmp_path, 'pwil', ['algorithm=PWIL', 'seed=3'] + (short or COMMON))
  err = capsys.readouterr().err
  assert err.count('[train_all]') == 1 and 'one after another' in err and 'algorithm=PWIL has no population launches' in err
  assert sorted(os.listdir(root)) == ENVS and np.isfinite(list(scores.values())).all() and worst == min(scores.values())
  for env in ENVS:
    assert {'agent.pth', 'metrics.pth'} <= set(os.listdir(os.path.join(root, env)))
