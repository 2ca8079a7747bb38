"""`-m gpu`: seed sweeps of GAIL with `imitation.loss_function=Mixup` as one population. The entry point (`il_gail_mixup_step_population`: the coefficient launch
k_gail_mix_fill_pop for mixup_alpha != 1, then k_gail_grad_pop with the learners' il_gail_extra array, k_gail_reduce and k_gail_reward, csrc/gail.hip) against
`il_noise_fill_beta` -> `il_gail_disc_step(extra)` -> `il_gail_reward` per learner, bit for bit over three updates, and against oracle/gail.py by value; its refusals;
`il.BatchedPopulationPlan` of Mixup learners against `plan.run()` per learner; and `python train.py -m seed=... algorithm=GAIL imitation.loss_function=Mixup
+sweep.gail_mixup_population=true` under both sweep schedules and as single train() runs, which must leave the same bytes. The bodies also run on the host emulation of
the kernels (tests/test_population_gail_mixup_emulated.py)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import inputs as gi
from oracle import gail as ogail

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib
  from imitation_learning_amd import memory as il_memory
  from imitation_learning_amd import training as il_training
  from gpu_util import DEV, N, T, Cfg, close_params, fill_memory

KEY = '+sweep.gail_mixup_population=true'
UPDATES = 3
LR, WD = 3e-4, 10.0


# ---------------------------------------------------------------------------------------------
# The cases: a pairwise-covering subset of the factors below (every value of every factor beside every value of every other factor at least once), built greedily in a
# fixed order, so the list is the same in every process. B: 16 = one tile (tiles per workgroup clipped to 1), 48 = three tiles in one workgroup, 80 = a workgroup of four
# tiles and one of one tile (the early `tile + 1 >= nt` exit). grad_penalty 0: the Mixup call alone (one call); > 0: the gradient-penalty call beside it.
# ---------------------------------------------------------------------------------------------
FACTORS = (('B', (16, 48, 80)), ('dims', ((3, 1, False), (11, 3, False), (18, 6, False), (18, 6, True))), ('H', (64, 128)), ('sn', (True, False)), ('ent', (0.0, 0.24)),
           ('gp', (0.0, 1.0)), ('alpha', (1.0, 0.4, 2.5)), ('L', (1, 3, 9)))


def _pairwise(factors):
  sizes = [len(v) for _, v in factors]
  todo = {(i, a, j, b) for i, j in itertools.combinations(range(len(sizes)), 2) for a in range(sizes[i]) for b in range(sizes[j])}
  rows = []
  while todo:
    best, gain = None, -1
    for cand in itertools.product(*[range(n) for n in sizes]):   # 3456 candidates: the row that covers the most pairs still open, the first such in lexicographic order
      g = sum((i, cand[i], j, cand[j]) in todo for i, j in itertools.combinations(range(len(sizes)), 2))
      if g > gain: best, gain = cand, g
    rows.append(best)
    todo -= {(i, best[i], j, best[j]) for i, j in itertools.combinations(range(len(sizes)), 2)}
  return [{name: values[k] for (name, values), k in zip(factors, row)} for row in rows]


def _case_id(c):
  S, A, so = c['dims']
  return f'B{c["B"]}-S{S}-A{A}{"-state_only" if so else ""}-H{c["H"]}-{"sn" if c["sn"] else "plain"}-ent{c["ent"]}-gp{c["gp"]}-alpha{c["alpha"]}-L{c["L"]}'


CASES = _pairwise(FACTORS)
assert 12 <= len(CASES) <= 24, len(CASES)


def _icfg(c, loss='Mixup'):
  return Cfg(state_only=c['dims'][2], spectral_norm=c['sn'], loss_function=loss, grad_penalty=c['gp'], entropy_bonus=c['ent'], mixup_alpha=c['alpha'], pos_class_prior=0.7,
             nonnegative_margin=float('inf'), discriminator=Cfg(hidden_size=c['H'], depth=1, activation='relu', reward_shaping=False, subtract_log_policy=False, reward_function='AIRL'))


class _Learner:
  """One discriminator with everything it owns: parameters, AdamW moments and step, u / v buffers (disc.sn), gradient arena, Philox key, update counter, the two
  batches, its reward buffer and its coefficient buffer."""


def _learners(c, seed, loss='Mixup'):
  S, A, so = c['dims']
  B, out = c['B'], []
  for l in range(c['L']):
    ln = _Learner()
    torch.manual_seed(1000 * seed + l)
    rs = np.random.RandomState(1000 * seed + l)
    ln.icfg = _icfg(c, loss)
    ln.disc = il.GAILDiscriminator(S, A, ln.icfg, 0.97, device=DEV)
    ln.opt = il.AdamW(ln.disc, lr=LR, weight_decay=WD)
    n = ln.opt.exp_avg.numel()
    ln.opt.exp_avg.copy_(T((1e-3 * rs.standard_normal(n)).astype(np.float32))); ln.opt.exp_avg_sq.copy_(T((1e-6 * rs.uniform(0.5, 1.5, n)).astype(np.float32)))
    ln.opt.step_count[0] = 2 + l   # every learner at its own optimiser step
    ln.d = il_training.disc_descriptor(ln.disc, B, ln.opt, ln.icfg, tag=('gail-mixup-population', seed, l))
    ln.key = 90001 + 7919 * l
    ln.ctr = torch.tensor([5 + 3 * l], dtype=torch.int32, device=DEV)   # every learner at its own update counter
    ln.d.noise_seed, ln.d.noise_counter = ln.key, ln.ctr.data_ptr()
    ln.pol = {k: T(v) for k, v in gi.transitions(rs, B, S, A, weighted=True).items()}
    ln.exp = {k: T(v) for k, v in gi.transitions(rs, B, S, A, state_shift=0.5, weighted=True).items()}
    ln.pb, ln.eb = il_memory.batch_desc(ln.pol), il_memory.batch_desc(ln.exp)
    ln.rewards = torch.full((B,), -7.5, device=DEV)
    ln.eps = torch.full((B,), -7.5, device=DEV)
    out.append(ln)
  return out


def _snapshot(learners):
  """(parameters, m, v, optimiser step, gradient arena, rewards, coefficients, update counter, u / v buffers) per learner."""
  torch.cuda.synchronize()
  return [[N(ln.disc.flat), N(ln.opt.exp_avg), N(ln.opt.exp_avg_sq), N(ln.opt.step_count[:1]), N(ln.opt.grad), N(ln.rewards), N(ln.eps), N(ln.ctr), N(ln.disc.sn)] for ln in learners]


NAMES = ('parameters', 'm', 'v', 'optimiser step', 'gradient arena', 'rewards', 'eps_mix', 'update counter', 'spectral-norm u / v buffers')


def _bump(learners):
  for ln in learners: ln.ctr.add_(1)   # what the actor step of the learner's SAC update does between two discriminator steps


def _per_learner(learners, alpha):
  """The reference: il_noise_fill_beta -> il_gail_disc_step(extra) -> il_gail_reward, one learner after the other; UPDATES updates, a snapshot after each."""
  L_, st, out = _lib.lib(), _lib.stream_ptr(), []
  for _ in range(UPDATES):
    for ln in learners:
      extra = None
      if alpha != 1.0:
        _lib.check(L_.il_noise_fill_beta(C.c_uint64(ln.key), _lib.ptr(ln.ctr), alpha, ln.eps.numel(), _lib.ptr(ln.eps), st))
        extra = C.byref(_lib.GailExtra(eps_mix=ln.eps.data_ptr()))
      _lib.check(L_.il_gail_disc_step(C.byref(ln.d), C.byref(ln.pb), C.byref(ln.eb), None, extra, 0, st))
      _lib.check(L_.il_gail_reward(C.byref(ln.d), C.byref(ln.pb), _lib.ptr(ln.rewards), None, None, st))
    out.append(_snapshot(learners))
    _bump(learners)
  return out


def _population_args(learners, alpha, with_extras=None):
  """(positional arguments of il_gail_mixup_step_population in front of the stream, what keeps their memory alive)."""
  with_extras = alpha != 1.0 if with_extras is None else with_extras
  descs = il_training._device_array([ln.d for ln in learners], DEV)
  pol, exp = il_training._device_array([ln.pb for ln in learners], DEV), il_training._device_array([ln.eb for ln in learners], DEV)
  rewards = torch.tensor([ln.rewards.data_ptr() for ln in learners], dtype=torch.int64, device=DEV)
  extras = [_lib.GailExtra(eps_mix=ln.eps.data_ptr()) for ln in learners]
  host = (_lib.GailExtra * len(learners))(*extras)
  dev = il_training._device_array(extras, DEV)
  args = [_lib.ptr(descs), _lib.ptr(pol), _lib.ptr(exp), _lib.ptr(rewards), len(learners), C.byref(learners[0].d), _lib.ptr(dev) if with_extras else None,
          C.cast(host, C.c_void_p) if with_extras else None, alpha]
  return args, (descs, pol, exp, rewards, host, dev)


def _population(learners, alpha):
  args, keep = _population_args(learners, alpha)
  out = []
  for _ in range(UPDATES):
    _lib.check(_lib.lib().il_gail_mixup_step_population(*args, _lib.stream_ptr()))
    out.append(_snapshot(learners))
    _bump(learners)
  return out


@pytest.mark.parametrize('c', [pytest.param(c, id=_case_id(c)) for c in CASES])
def test_mixup_step_population_equals_the_per_learner_sequence(c):
  """One il_gail_mixup_step_population for L learners against L sequences il_noise_fill_beta -> il_gail_disc_step(extra) -> il_gail_reward, three updates in a row with
  every learner's update counter bumped in between: parameters, m, v, optimiser step, the u / v buffers, the gradient arena, the rewards and (alpha != 1) the eps_mix
  buffers equal bit for bit after every update. Learners differ in everything they own - parameters, moments, step, key, counter, batches - so a workgroup that read
  another learner's descriptor, extra or counter fails; and the learners' results differ from each other."""
  want = _per_learner(_learners(c, 3), c['alpha'])
  got = _population(_learners(c, 3), c['alpha'])
  for u in range(UPDATES):
    for l in range(c['L']):
      for name, a, b in zip(NAMES, want[u][l], got[u][l]):
        if name == 'eps_mix' and c['alpha'] == 1.0:
          assert (b == -7.5).all(), 'alpha = 1 draws on chip: nobody writes the buffer'
          continue
        assert np.isfinite(a.astype(np.float64)).all(), (u, l, name)
        np.testing.assert_array_equal(a, b, err_msg=f'update {u}, learner {l} of {c["L"]}: {name}')
      assert int(got[u][l][3][0]) == 2 + l + u + 1 and int(got[u][l][7][0]) == 5 + 3 * l + u
      if c['alpha'] != 1.0: assert (got[u][l][6] >= 0).all() and (got[u][l][6] <= 1).all() and (u == 0 or not np.array_equal(got[u][l][6], got[u - 1][l][6])), 'new Beta draws inside [0, 1] (float32 rounds a draw next to 1 to 1) every update'
    for l in range(1, c['L']):
      assert not np.array_equal(got[u][0][0], got[u][l][0]) and not np.array_equal(got[u][0][5], got[u][l][5]), 'the learners are meant to differ'
  assert not np.array_equal(got[0][0][0], got[UPDATES - 1][0][0]), 'the updates are meant to move the parameters'
  assert c['sn'] == (not np.array_equal(got[0][0][8], got[UPDATES - 1][0][8])), 'the power iterations move u / v (spectral norm on), or nothing touches them'


def _noise(key, counter, stream_id, n):
  out = torch.empty(n, device=DEV)
  _lib.check(_lib.lib().il_noise_fill(C.c_uint64(key), counter, stream_id, n, _lib.ptr(out), _lib.stream_ptr()))
  torch.cuda.synchronize()
  return N(out)


@pytest.mark.parametrize('alpha', [1.0, 0.4])
def test_mixup_step_population_against_the_oracle(alpha):
  """Every learner's step is oracle/gail.py's Mixup step (pinned to the reference) on its rows with its coefficients - the Mixup stream's U(0,1) of its key and counter for
  alpha = 1, its eps_mix buffer otherwise - and the gradient-penalty uniforms of the same key and counter; held to the single-learner test's bound
  (tests/test_gpu_parity.py::test_update_plan_mixup_with_beta_coefficients_drawn_on_the_device: close_params(..., lr, k + 1) with one Adam step of slack per update)."""
  c = dict(B=48, dims=(18, 6, False), H=64, sn=True, ent=0.05, gp=1.0, alpha=alpha, L=3)
  learners = _learners(c, 5)
  cat = lambda t: np.concatenate([N(t['states']), N(t['actions'])], axis=1)
  oracles = []
  for ln in learners:
    ods = ogail.DiscState(ln.disc.in_dim, c['H'], True)
    ods.unpack_into(N(ln.disc.flat)); v = ln.disc.views()
    for kk in ('u1', 'v1', 'u2', 'v2'): getattr(ods, kk)[...] = N(v[kk])
    oracles.append((ods, None))
  for ln in learners:   # the oracle's optimiser (DiscState.m, v, t) starts from zero moments at step 0: so do these learners
    ln.opt.exp_avg.zero_(); ln.opt.exp_avg_sq.zero_(); ln.opt.step_count[0] = 0
  args, keep = _population_args(learners, alpha)
  for k in range(UPDATES):
    _lib.check(_lib.lib().il_gail_mixup_step_population(*args, _lib.stream_ptr()))
    torch.cuda.synchronize()
    for l, (ln, (ods, _)) in enumerate(zip(learners, oracles)):
      counter = 5 + 3 * l + k
      eps = _noise(ln.key, counter, 7, c['B']) if alpha == 1.0 else N(ln.eps)   # 7: IL_STREAM_MIX
      assert (eps >= 0).all() and (eps <= 1).all()
      ogail.gail_update(ods, cat(ln.pol), N(ln.pol['weights']), cat(ln.exp), N(ln.exp['weights']), _noise(ln.key, counter, 3, c['B']), lr=LR, weight_decay=WD, grad_penalty=1.0,
                        entropy_bonus=0.05, loss_function='Mixup', eps_mix=eps)
      close_params(N(ln.disc.flat)[:ods.pack().size], ods.pack(), f'mixup population alpha {alpha}: learner {l} after update {k + 1}', LR, k + 1)
    _bump(learners)


def test_mixup_step_population_refusals():
  """Every refusal is IL_ERR_ARG with a text naming the entry point, and nothing is launched (parameters, rewards and coefficient buffers stay as they were); the same
  arrays are served once the call is valid. il_gail_step_population keeps refusing Mixup with its present text."""
  L_ = _lib.lib()
  c = dict(B=16, dims=(11, 3, False), H=64, sn=True, ent=0.0, gp=1.0, alpha=0.4, L=2)
  learners = _learners(c, 7)
  before = _snapshot(learners)
  args, keep = _population_args(learners, 0.4)
  st = _lib.stream_ptr()

  def refused(a, word):
    assert L_.il_gail_mixup_step_population(*a, st) == 1, word   # IL_ERR_ARG
    err = L_.il_last_error()
    assert b'il_gail_mixup_step_population' in err and word in err, (word, err)

  def swap(i, v):
    a = list(args); a[i] = v
    return a
  for loss, word in (('BCE', b'not Mixup'), ('PUGAIL', b'not Mixup')):   # a shape_host whose loss is not Mixup
    other = _learners(dict(c, L=1), 7, loss=loss)[0]
    refused(swap(5, C.byref(other.d)), word)
  clamped = _learners(dict(c, L=1), 7)[0]
  clamped.d.pu_clamped, clamped.d.nonnegative_margin = 1, 0.05
  refused(swap(5, C.byref(clamped.d)), b'pu_clamped')
  for alpha in (0.0, -1.0, float('nan')):
    refused(swap(8, alpha), b'must be > 0')
  refused(swap(7, None)[:6] + [None, None, 0.4], b'needs the il_gail_extra array')   # alpha != 1 without an extras array
  refused(swap(7, None), b'device array and its host copy')
  refused(swap(6, None), b'device array and its host copy')
  for field in ('logit_offset_policy', 'logit_offset_expert', 'logit_offset_mix'):   # subtract_log_policy has no population form
    host = (_lib.GailExtra * 2)(_lib.GailExtra(eps_mix=learners[0].eps.data_ptr()), _lib.GailExtra(eps_mix=learners[1].eps.data_ptr()))
    setattr(host[1], field, learners[1].eps.data_ptr())
    refused(swap(7, C.cast(host, C.c_void_p)), b'learner 1 carries a logit offset')
    refused(swap(8, 1.0)[:7] + [C.cast(host, C.c_void_p), 1.0], b'learner 1 carries a logit offset')   # ... at alpha = 1 as well
  host = (_lib.GailExtra * 2)(_lib.GailExtra(eps_mix=learners[0].eps.data_ptr()), _lib.GailExtra())
  refused(swap(7, C.cast(host, C.c_void_p)), b'learner 1 has no eps_mix buffer')
  for n in (0, -1, 65536):
    refused(swap(4, n), b'n_learners=')
  for i in (0, 1, 2, 3):
    refused(swap(i, None), b'null')
  after = _snapshot(learners)
  for a_l, b_l in zip(before, after):
    for a, b in zip(a_l, b_l): np.testing.assert_array_equal(a, b, err_msg='a refused call launched a kernel')
  # il_gail_step_population: as before
  assert L_.il_gail_step_population(*args[:6], st) == 1
  assert b'il_gail_step_population: loss_function Mixup is not available on the population path' in L_.il_last_error()
  assert all((a == b).all() for a_l, b_l in zip(before, _snapshot(learners)) for a, b in zip(a_l, b_l))
  # ... and the valid call is served: the per-learner sequence's bits
  _lib.check(L_.il_gail_mixup_step_population(*args, st))
  got = _snapshot(learners)
  want = _per_learner(_learners(c, 7), 0.4)[0]
  for a_l, b_l in zip(want, got):
    for a, b in zip(a_l, b_l): np.testing.assert_array_equal(a, b)
  assert not np.array_equal(got[0][0], before[0][0])


# ---------------------------------------------------------------------------------------------
# il.BatchedPopulationPlan of Mixup learners against plan.run() per learner
# ---------------------------------------------------------------------------------------------
def _mixup_plans(n, alpha, B=64, loss='Mixup', alphas=None, **variant):
  """n independent GAIL learners whose loss is Mixup (own networks, rings, index streams, Philox keys and counters) as UpdatePlans at hopper dims, reproducibly - built like
  tests/test_gpu_parity.py::_population_learners builds its BCE learners."""
  il_training._NOISE.clear(); il_training._WS.clear()
  plans, nets_all = [], []
  S, A = gi.DIMS['hopper']
  for l in range(n):
    torch.manual_seed(40 + l)
    cfg = Cfg(hidden_size=64, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(40 + l)
    mem = il.ReplayMemory(4000, S, A, True, device=DEV); fill_memory(mem, gi.transitions(rs, 1500, S, A), 1500)
    emem = il.ReplayMemory(600, S, A, True, device=DEV); fill_memory(emem, gi.transitions(rs, 600, S, A, state_shift=0.5), 600)
    mem.index_rng = il.IndexStream(100 + l)
    icfg = Cfg(state_only=False, spectral_norm=True, loss_function=loss, grad_penalty=1.0, entropy_bonus=0.05, mixup_alpha=alphas[l] if alphas else alpha, pos_class_prior=0.7,
               nonnegative_margin=variant.get('margin', float('inf')),
               discriminator=Cfg(hidden_size=64, depth=variant.get('depth', 1), activation=variant.get('activation', 'relu'), reward_shaping=variant.get('reward_shaping', False),
                                 subtract_log_policy=variant.get('subtract_log_policy', False), reward_function='AIRL'))
    disc = il.GAILDiscriminator(S, A, icfg, 0.97, device=DEV)
    do = il.AdamW(disc, lr=3e-4, weight_decay=10)
    plans.append(il.UpdatePlan('GAIL', actor, critic, log_alpha, target, mem, ao, co, to, B, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=disc,
                               discriminator_optimiser=do, imitation_cfg=icfg, overlap=False, learner_id=l))
    nets_all.append((actor, critic, target, log_alpha, disc))
  return plans, nets_all


def _plans_state(plans, nets_all):
  torch.cuda.synchronize()
  return [[N(n.flat if hasattr(n, 'flat') else n) for n in nets] + [N(p.idx), N(p.eidx), N(p.logp), N(p.rewards)] for nets, p in zip(nets_all, plans)]


def _beta_draws(key, counter, alpha, n):
  ctr, out = torch.tensor([counter], dtype=torch.int32, device=DEV), torch.empty(n, device=DEV)
  _lib.check(_lib.lib().il_noise_fill_beta(C.c_uint64(key), _lib.ptr(ctr), alpha, n, _lib.ptr(out), _lib.stream_ptr()))
  torch.cuda.synchronize()
  return N(out)


def mixup_population_plan_equals_plan_run_per_learner(alpha, how, side):
  n, B = 3, 64
  plans, nets = _mixup_plans(n, alpha)
  want = []
  for _ in range(UPDATES):
    for p in plans: p.run()
    want.append(_plans_state(plans, nets))
  plans, nets = _mixup_plans(n, alpha)
  pop = il.BatchedPopulationPlan(plans)
  assert pop.algorithm == 'GAIL' and pop.mixup_alpha == alpha and (pop.side is not None) == side and (pop.extras is not None) == (alpha != 1.0)
  for u in range(UPDATES):
    if how == 'captured' and u > 0: pop.replay()
    else: pop.run()
    if how == 'captured' and u == 0:
      torch.cuda.synchronize()
      pop.capture()
    got = _plans_state(plans, nets)
    for l in range(n):
      for i, (a, b) in enumerate(zip(want[u][l], got[l])):
        assert np.isfinite(a.astype(np.float64)).all()
        np.testing.assert_array_equal(a, b, err_msg=f'update {u}, learner {l}, tensor {i}')
      if alpha != 1.0:   # after update u the buffer holds the Mixup stream's Beta draws of the learner's key at counter u
        np.testing.assert_array_equal(N(plans[l].eps_mix), _beta_draws(int(plans[l].disc.noise_seed), u, alpha, B), err_msg=f'update {u}, learner {l}: eps_mix')
    assert not np.array_equal(got[0][0], got[1][0]) and not np.array_equal(got[0][4], got[1][4]) and not np.array_equal(got[0][8], got[1][8]), 'the learners are meant to differ'
  assert len({int(p.disc.noise_seed) for p in plans}) == n


@pytest.mark.parametrize('how', ['eager', 'captured'])
@pytest.mark.parametrize('alpha', [1.0, 0.4])
def test_mixup_population_plan_equals_plan_run_per_learner(alpha, how):
  """Three updates of three Mixup learners at B = 64: BatchedPopulationPlan (eager; or one eager run, capture(), two replays), its discriminator launches on the side stream,
  against plan.run() per learner - actor, critic, target, log_alpha, discriminator, both index draws, log-probs and rewards bit for bit after every update; after update k
  learner l's eps_mix is il_noise_fill_beta(key_l, k, alpha)."""
  mixup_population_plan_equals_plan_run_per_learner(alpha, how, side=True)


@pytest.mark.parametrize('how', ['eager', 'captured'])
@pytest.mark.parametrize('alpha', [1.0, 0.4])
def test_mixup_population_plan_on_one_stream_equals_plan_run_per_learner(alpha, how, monkeypatch):
  """The same with IL_POP_OVERLAP=0: the discriminator launches in stream order in front of the SAC launches."""
  monkeypatch.setenv('IL_POP_OVERLAP', '0')
  mixup_population_plan_equals_plan_run_per_learner(alpha, how, side=False)


def test_mixup_population_plan_refusals():
  """Learners of different mixup_alpha or loss_function are refused by the plan; the in-plan variants keep raising where they did."""
  with pytest.raises(AssertionError, match='share mixup_alpha'):
    il.BatchedPopulationPlan(_mixup_plans(2, None, alphas=[0.4, 2.5])[0])
  with pytest.raises(AssertionError, match='share mixup_alpha'):
    il.BatchedPopulationPlan(_mixup_plans(2, None, alphas=[1.0, 0.4])[0])
  mixed = _mixup_plans(1, 1.0, loss='BCE')[0] + _mixup_plans(1, 1.0)[0]   # (never run: only their descriptors are looked at)
  with pytest.raises(AssertionError, match='share loss_function'):
    il.BatchedPopulationPlan(mixed)
  for variant in (dict(reward_shaping=True), dict(depth=2), dict(activation='tanh'), dict(subtract_log_policy=True)):
    with pytest.raises(NotImplementedError, match='a population of GAIL learners'):
      _mixup_plans(1, 0.4, **variant)
  with pytest.raises(NotImplementedError, match='a population of GAIL learners'):
    _mixup_plans(1, 1.0, loss='PUGAIL', margin=0.05)
  pop = il.BatchedPopulationPlan(_mixup_plans(2, 1.0, loss='BCE')[0])   # BCE learners: il_gail_step_population, as before
  assert pop.mixup_alpha is None and pop.extras is None


# ---------------------------------------------------------------------------------------------
# train.py -m seed=... algorithm=GAIL imitation.loss_function=Mixup +sweep.gail_mixup_population=true
# ---------------------------------------------------------------------------------------------
from test_train_gpu import COMMON  # noqa: E402  (steps 260, batch 64, two evaluations of two episodes, 60-step episodes)

MIXUP_RUN = ['algorithm=GAIL', 'env=hopper', 'imitation.loss_function=Mixup']
GAIL_10_DISC = ['imitation.spectral_norm=false', 'imitation.discriminator.hidden_size=64', 'imitation.discriminator.reward_function=AIRL', 'imitation.grad_penalty=0.4359957529231906',
                'imitation.entropy_bonus=0.024794470891356467']   # the GAIL_10_trajectories overlay's discriminator settings (no spectral norm) at the short runs' batch of 64
SWEEP_CASES = [pytest.param([], id='alpha1'), pytest.param(['imitation.mixup_alpha=0.5'], id='alpha0.5'), pytest.param(GAIL_10_DISC, id='GAIL_10-discriminator-no-spectral-norm')]


def _single(tmp_path, name, seed, extra, short):
  """One train() of one seed in its own directory, from fresh process-wide update counters."""
  if ROOT not in sys.path: sys.path.insert(0, ROOT)
  import train
  from imitation_learning_amd import config
  il_training._NOISE.clear(); il_training._WS.clear()
  d = tmp_path / name
  d.mkdir()
  before = os.getcwd()
  os.chdir(d)
  try:
    train.train(config.compose(MIXUP_RUN + [f'seed={seed}'] + list(extra) + short))
  finally:
    os.chdir(before)
  return {f: torch.load(d / f, weights_only=False) for f in ('agent.pth', 'discriminator.pth', 'metrics.pth')}


def mixup_sweep_schedules_and_single_runs_leave_the_same_bytes(tmp_path, capsys, extra, short, tp, min_updates=2):
  """`-m seed=3,4` with the opt-in key under +sweep.schedule=population and per_learner, and train() of seed 3 and of seed 4: the same bytes in agent.pth, discriminator.pth
  and metrics.pth (timing keys aside) three times; each sweep announces one population of 2 learners; the jobs differ from each other. `tp`: tests/test_population_acting_gpu.py."""
  argv = ['-m', 'seed=3,4'] + MIXUP_RUN + [KEY] + short + extra
  jobs = {}
  for schedule in ('population', 'per_learner'):
    capsys.readouterr()
    root, scores = tp._sweep(tmp_path, schedule, argv + [f'+sweep.schedule={schedule}'])
    err = capsys.readouterr().err
    assert err.count('[train] sweep:') == 1 and 'train as one population of 2 learners' in err and f'+sweep.schedule={schedule}' in err and 'il_gail_mixup_step_population' in err, err
    assert np.isfinite(scores).all() and sorted(os.listdir(root)) == ['0', '1']
    jobs[schedule] = [tp._job_files(root, j) for j in (0, 1)]
  jobs['single'] = [_single(tmp_path, f'single{seed}', seed, extra, short) for seed in (3, 4)]
  for j in (0, 1):
    fp = jobs['population'][j]
    assert set(fp) == {'agent.pth', 'discriminator.pth', 'metrics.pth'}
    m = fp['metrics.pth']
    assert len(m['update_steps']) >= min_updates and len(m['test_steps']) == 2 and all(np.isfinite(q).all() for q in m['Q_values']) and all(np.isfinite(r).all() for r in m['predicted_rewards'])
    for other in ('per_learner', 'single'):
      fo = jobs[other][j]
      assert set(fo) == set(fp)
      for f in fp:
        a, b = ({k: v for k, v in x.items() if k not in tp.TIMING_KEYS} for x in (fp[f], fo[f]))
        tp._assert_same_nested(a, b, f'job {j}: {f}: population against {other}')
  a0, a1 = (jobs['population'][j]['agent.pth']['actor'] for j in (0, 1))
  assert any(not torch.equal(v, a1[k]) for k, v in a0.items()), 'the jobs of a seed sweep are meant to differ'
  d0, d1 = (jobs['population'][j]['discriminator.pth'] for j in (0, 1))
  assert any(not torch.equal(v, d1[k]) for k, v in d0.items() if torch.is_tensor(v))


@pytest.mark.parametrize('extra', SWEEP_CASES)
def test_mixup_seed_sweep_population_equals_per_learner_equals_single_runs(tmp_path, capsys, extra):
  import test_population_acting_gpu as tp
  mixup_sweep_schedules_and_single_runs_leave_the_same_bytes(tmp_path, capsys, extra, COMMON, tp)
