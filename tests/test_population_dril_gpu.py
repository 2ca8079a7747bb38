"""`-m gpu`: seed sweeps of DRIL as one population. The reward launch (`il_dril_reward_population`: k_dril_unc_population, csrc/dril.hip) against one `il_dril_uncertainty`
per learner, bit for bit, and its refusals; the behavioural-cloning auxiliary launch (`il_bc_step_population`, csrc/sac.hip) against one `il_bc_step` per learner, bit for
bit, and its refusals; `il.BatchedPopulationPlan('DRIL')` with and without `bc_aux` against `plan.run()` per learner; and `python train.py -m seed=... algorithm=DRIL` under
both sweep schedules, which must leave the same bytes. The bodies also run on the host emulation of the kernels (tests/test_population_dril_emulated.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import inputs as gi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib
  from imitation_learning_amd import training as il_training
  from gpu_util import DEV, N, T, Cfg, fill_memory

GUARD, SENTINEL = 32, -7.5   # guard floats on both sides of every learner's output buffers
OFFSET = 0x40000000          # the noise offset UpdatePlan('DRIL') passes
IL_ERR_ARG, IL_ERR_UNSUPPORTED, IL_ERR_WORKSPACE = 1, 2, 4

# (S, A, H, depth, activation, B, L, p_in, p)
SHIPPED = (11, 3, 64, 1, 'tanh', 20, 3, 0.1, 0.1)        # conf/algorithm/DRIL.yaml's ensemble: 20 rows leave the third 8-row tile half empty
DRIL_25 = (17, 6, 32, 2, 'relu', 16, 2, 0.40, 0.55)      # DRIL_25_trajectories' shape: depth 2, relu, heavy dropout
NO_DROPOUT = (11, 3, 64, 1, 'tanh', 5, 1, 0.0, 0.0)      # one learner, less than one tile, no dropout: five equal ensemble members
LIMIT = (128, 8, 256, 2, 'relu', 8, 2, 0.1, 0.1)         # the limit width: 105920 bytes of LDS, the > 64 KiB opt-in of the new kernel
KERNEL_CASES = [pytest.param(SHIPPED, id='shipped'), pytest.param(DRIL_25, id='DRIL_25-relu-depth2'), pytest.param(NO_DROPOUT, id='no-dropout-one-learner'),
                pytest.param(LIMIT, id='limit-width')]


def _dril_population(case, seed=0):
  """L ensembles of one shape - own random parameters, own batch, own Philox key (the process seed while the descriptor is built) and own non-zero device counter - as
  (descriptors, batch descriptors, keep). The weights are fan-in scaled and the head is small (means near 0, log standard deviations near 0.3), the actions stay inside
  (-0.8, 0.8): exp(log_prob) is then around exp(-1.5 A) and nowhere near underflow."""
  S, A, H, depth, activation, B, L, p_in, p = case
  mcfg = Cfg(hidden_size=H, depth=depth, activation=activation, input_dropout=p_in, dropout=p)
  rs = np.random.RandomState(4321 + seed)
  descs, batches, keep = [], [], []
  for l in range(L):
    torch.manual_seed(700 + 13 * l)
    d = il.DropoutSoftActor(S, A, mcfg, device=DEV)
    lay = [(H, S)] + [(H, H)] * (depth - 1)
    parts = [np.concatenate([(rs.standard_normal(o * i) / np.sqrt(i)).astype(np.float32), (0.1 * rs.standard_normal(o)).astype(np.float32)]) for o, i in lay]
    head_b = np.concatenate([0.1 * rs.standard_normal(A), 0.3 + 0.05 * rs.standard_normal(A)]).astype(np.float32)
    parts.append(np.concatenate([(0.3 * rs.standard_normal(2 * A * H) / np.sqrt(H)).astype(np.float32), head_b]))
    d.flat.copy_(T(np.concatenate(parts)))
    d.q = 0.0
    tr = gi.transitions(rs, B, S, A)
    tr['actions'] = (0.8 * tr['actions']).astype(np.float32)
    tr = {k: T(v) for k, v in tr.items() if k in ('states', 'actions', 'rewards', 'next_states', 'terminals', 'weights', 'absorbing')}
    counter = torch.tensor([3 + 5 * l], dtype=torch.int32, device=DEV)
    desc, b = d._desc(B), il.memory.batch_desc(tr)
    desc.noise_counter = counter.data_ptr()
    assert (desc.p_in, desc.p) == (np.float32(p_in), np.float32(p)) and desc.noise_seed == 700 + 13 * l
    descs.append(desc); batches.append(b); keep.append((d, tr, counter))
  return descs, batches, keep


def _guarded(L, B):
  bufs = [torch.full((GUARD + B + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(L)]
  ptrs = torch.tensor([b[GUARD:].data_ptr() for b in bufs], dtype=torch.int64, device=DEV)
  return bufs, ptrs


def _per_learner(descs, batches, B):
  """(uncertainties, rewards) per learner by il_dril_uncertainty under the descriptor as it stands."""
  out = []
  for desc, b in zip(descs, batches):
    u, r = (torch.full((B,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2))
    _lib.check(_lib.lib().il_dril_uncertainty(C.byref(desc), C.byref(b), None, None, None, OFFSET, _lib.ptr(u), _lib.ptr(r), _lib.stream_ptr()))
    out.append((u, r))
  torch.cuda.synchronize()
  return out


def _with_median_thresholds(descs, batches, B):
  """Every learner's q <- the median of its own reference uncertainties (both reward signs then occur); returns the reference under those thresholds."""
  for desc, (u, _) in zip(descs, _per_learner(descs, batches, B)):
    desc.q = float(np.median(N(u)))
  return _per_learner(descs, batches, B)


@pytest.mark.parametrize('case', KERNEL_CASES)
def test_dril_reward_population_equals_il_dril_uncertainty_per_learner(case):
  """One launch for L learners against L calls of il_dril_uncertainty: torch.equal per learner for uncertainties and rewards, guard floats untouched. The host descriptor
  is learner 0's, so a kernel that took the parameters, the threshold, the Philox key or the counter from it instead of from the learner's device descriptor fails for
  every other learner; the counters are non-zero and differ, so one that ignored them fails for all."""
  S, A, H, depth, activation, B, L, p_in, p = case
  descs, batches, keep = _dril_population(case)
  want = _with_median_thresholds(descs, batches, B)
  ubufs, uptrs = _guarded(L, B)
  rbufs, rptrs = _guarded(L, B)
  d_dev, b_dev = il_training._device_array(descs, DEV), il_training._device_array(batches, DEV)
  _lib.check(_lib.lib().il_dril_reward_population(_lib.ptr(d_dev), _lib.ptr(b_dev), _lib.ptr(rptrs), _lib.ptr(uptrs), L, C.byref(descs[0]), OFFSET, _lib.stream_ptr()))
  torch.cuda.synchronize()
  for l in range(L):
    wu, wr = want[l]
    assert torch.isfinite(wu).all() and float(wu.min()) >= 0.0, f'learner {l}: the reference uncertainties are variances'
    assert bool(((wr == 1.0) | (wr == -1.0)).all())
    if p > 0:
      distinct = set(N(wu).tolist()) - {0.0}
      assert len(distinct) > B // 2, f'learner {l}: the reference uncertainties are meant to vary ({len(distinct)} distinct non-zero values of {B})'
      assert bool((wr == 1.0).any()) and bool((wr == -1.0).any()), f'learner {l}: under the median threshold both reward signs occur'
    else:   # five equal members: an exact zero variance, and +1 everywhere at q = 0
      assert bool((wu == 0.0).all()) and descs[l].q == 0.0 and bool((wr == 1.0).all()), N(wu)
    for name, bufs, w in (('uncertainty', ubufs, wu), ('reward', rbufs, wr)):
      got = bufs[l][GUARD:GUARD + B]
      assert torch.equal(got, w), f'learner {l}: {name}: max |difference| {float((got - w).abs().max()):.3e}'
      assert bool((bufs[l][:GUARD] == SENTINEL).all()) and bool((bufs[l][GUARD + B:] == SENTINEL).all()), f'learner {l}: a guard float of the {name} buffer was written'
  for l in range(1, L):   # the learners really differ: another learner's parameters, batch, key, counter or threshold would not pass
    assert not torch.equal(want[0][0], want[l][0]) and descs[l].q != descs[0].q
    under_q0 = torch.where(want[l][0] <= descs[0].q, 1.0, -1.0)   # learner l's rewards under learner 0's threshold
    assert not torch.equal(under_q0, want[l][1])
  if p > 0:   # the counter and the key matter: the same ensembles at counter 0 / under learner 0's key give other uncertainties
    for l in range(L):
      moved = _lib.Dril.from_buffer_copy(descs[l]); moved.noise_counter = None
      assert not torch.equal(_per_learner([moved], [batches[l]], B)[0][0], want[l][0])
      if l > 0:
        rekeyed = _lib.Dril.from_buffer_copy(descs[l]); rekeyed.noise_seed = descs[0].noise_seed
        assert not torch.equal(_per_learner([rekeyed], [batches[l]], B)[0][0], want[l][0])
  # rewards alone (what BatchedPopulationPlan asks for): the uncertainty pointers may be NULL
  rbufs2, rptrs2 = _guarded(L, B)
  _lib.check(_lib.lib().il_dril_reward_population(_lib.ptr(d_dev), _lib.ptr(b_dev), _lib.ptr(rptrs2), None, L, C.byref(descs[0]), OFFSET, _lib.stream_ptr()))
  torch.cuda.synchronize()
  assert all(torch.equal(rbufs2[l], rbufs[l]) for l in range(L))


def _bare_dril(S, A, H, depth, activation, B, some, p_in=0.0, p=0.0):
  d = _lib.Dril()
  d.state_dim, d.action_dim, d.hidden, d.batch, d.depth, d.activation, d.p_in, d.p = S, A, H, B, depth, activation, p_in, p
  d.params = some.data_ptr()
  return d


def test_dril_reward_population_refusals():
  """Every refusal names il_dril and the offending value, and nothing is launched: the valid device arrays of a one-learner population stay behind every call, so a launch
  that went out anyway would write its rewards. (IL_ERR_UNSUPPORTED cannot be reached from outside: at the largest dims the shape check admits - state 128, hidden 256,
  depth 2 - the 40-row tile is 105920 bytes, below the 160 KiB a workgroup can have.)"""
  L_ = _lib.lib()
  S, A, H, depth, activation, B, L, p_in, p = NO_DROPOUT
  descs, batches, keep = _dril_population(NO_DROPOUT)
  ubufs, uptrs = _guarded(L, B)
  rbufs, rptrs = _guarded(L, B)
  d_dev, b_dev = il_training._device_array(descs, DEV), il_training._device_array(batches, DEV)
  dd, bb, rr, uu, ok = _lib.ptr(d_dev), _lib.ptr(b_dev), _lib.ptr(rptrs), _lib.ptr(uptrs), C.byref(descs[0])
  some = torch.zeros(64, dtype=torch.float32, device=DEV)
  bare = lambda *a, **k: C.byref(_bare_dril(*a, some, **k))
  for args, word in (((None, bb, rr, uu, L, ok), b'null device array'), ((dd, None, rr, uu, L, ok), b'null device array'), ((dd, bb, None, uu, L, ok), b'null device array'),
                     ((dd, bb, rr, uu, L, None), b'null shape'), ((dd, bb, rr, uu, 0, ok), b'n_learners=0'), ((dd, bb, rr, uu, 65536, ok), b'n_learners=65536'),
                     ((dd, bb, rr, uu, L, bare(11, 3, 64, 1, 0, 0)), b'batch=0'), ((dd, bb, rr, uu, L, bare(11, 3, 64, 1, 0, -8)), b'batch=-8'),
                     ((dd, bb, rr, uu, L, bare(129, 3, 64, 1, 0, B)), b'state=129'), ((dd, bb, rr, uu, L, bare(11, 9, 64, 1, 0, B)), b'action=9'),
                     ((dd, bb, rr, uu, L, bare(11, 3, 258, 1, 0, B)), b'hidden=258'), ((dd, bb, rr, uu, L, bare(11, 3, 63, 1, 0, B)), b'hidden=63'),
                     ((dd, bb, rr, uu, L, bare(11, 3, 64, 3, 0, B)), b'depth'), ((dd, bb, rr, uu, L, bare(11, 3, 64, 1, 2, B)), b'activation'),
                     ((dd, bb, rr, uu, L, bare(11, 3, 64, 1, 0, B, p=1.0)), b'dropout probabilities'), ((dd, bb, rr, uu, L, bare(11, 3, 64, 1, 0, B, p_in=-0.1)), b'dropout probabilities')):
    assert L_.il_dril_reward_population(*args, OFFSET, _lib.stream_ptr()) == IL_ERR_ARG, word
    assert b'il_dril' in L_.il_last_error() and word in L_.il_last_error(), (word, L_.il_last_error())
  torch.cuda.synchronize()
  assert all(bool((b == SENTINEL).all()) for b in ubufs + rbufs), 'a refused call launched its kernel'
  _lib.check(L_.il_dril_reward_population(dd, bb, rr, uu, L, ok, OFFSET, _lib.stream_ptr()))   # ... and the same arrays are served once the call is valid
  torch.cuda.synchronize()
  wu, wr = _per_learner(descs, batches, B)[0]
  assert torch.equal(ubufs[0][GUARD:GUARD + B], wu) and torch.equal(rbufs[0][GUARD:GUARD + B], wr)


# ---------------------------------------------------------------------------------------------
# il_bc_step_population against il_bc_step per learner
# ---------------------------------------------------------------------------------------------
# (S, A, H, B, L)
BC_CASES = [pytest.param((11, 3, 256, 32, 3), id='hopper-H256-B32-L3'), pytest.param((17, 6, 128, 48, 2), id='S17-A6-H128-B48-L2'), pytest.param((112, 8, 64, 16, 1), id='S112-A8-H64-one-tile-one-learner')]


def _bc_learners(shape, guard_loss=True):
  """L actors of one shape with their optimisers, il_sac descriptors (own workspace: learner_id as the scratch tag) and weighted expert batches, reproducibly."""
  S, A, H, B, L = shape
  il_training._NOISE.clear(); il_training._WS.clear()
  out = []
  for l in range(L):
    torch.manual_seed(900 + l)
    cfg = Cfg(hidden_size=H, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=1e-2), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(900 + l)
    tr = gi.transitions(rs, B, S, A, state_shift=0.25 * l, weighted=True)
    tr = {k: T(v) for k, v in tr.items() if k in ('states', 'actions', 'rewards', 'next_states', 'terminals', 'weights', 'absorbing')}
    sac = il_training.sac_descriptor(actor, critic, log_alpha, target, B, ao, co, to, 0.97, -0.5 * A, 0.99, tag=l, seed_offset=7919 * (l + 1))
    loss = torch.full((GUARD + B // 16 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    out.append(Cfg(actor=actor, critic=critic, target=target, log_alpha=log_alpha, ao=ao, co=co, to=to, tr=tr, eb=il.memory.batch_desc(tr), sac=sac, loss=loss))
  return out


def _bc_state(learners):
  torch.cuda.synchronize()
  return [[N(x.actor.flat), N(x.ao.exp_avg), N(x.ao.exp_avg_sq), N(x.ao.step_count[:1]), N(x.loss), N(x.critic.flat), N(x.target.flat), N(x.log_alpha), N(x.co.step_count[:1])] for x in learners]


@pytest.mark.parametrize('shape', BC_CASES)
def test_bc_step_population_equals_il_bc_step_per_learner(shape):
  """Two consecutive steps: one il_bc_step_population per step against one il_bc_step per learner and step - the actor arena, Adam's m, v and step count and the loss
  partials bit for bit (guard floats around the partials untouched); critics, targets, log alpha and the critic optimiser's step count do not move."""
  S, A, H, B, L = shape
  L_ = _lib.lib()
  ref = _bc_learners(shape)
  before = _bc_state(ref)
  for _ in range(2):
    for x in ref:
      od = x.ao.desc()
      _lib.check(L_.il_bc_step(_lib.ptr(x.actor.flat), _lib.ptr(x.ao.grad), C.byref(od), S, A, H, C.byref(x.eb), C.c_void_p(x.sac.workspace), x.sac.workspace_floats, _lib.ptr(x.loss[GUARD:]), 0,
                               _lib.stream_ptr()))
  want = _bc_state(ref)
  pop = _bc_learners(shape)
  d_dev, b_dev = il_training._device_array([x.sac for x in pop], DEV), il_training._device_array([x.eb for x in pop], DEV)
  loss_ptrs = torch.tensor([x.loss[GUARD:].data_ptr() for x in pop], dtype=torch.int64, device=DEV)
  for _ in range(2):
    _lib.check(L_.il_bc_step_population(_lib.ptr(d_dev), _lib.ptr(b_dev), L, C.byref(pop[0].sac), _lib.ptr(loss_ptrs), 0, _lib.stream_ptr()))
  got = _bc_state(pop)
  for l in range(L):
    for i, name in enumerate(('actor', 'exp_avg', 'exp_avg_sq', 'step', 'loss partials', 'critic', 'target', 'log_alpha', 'critic step')):
      assert np.isfinite(want[l][i].astype(np.float64)).all()
      np.testing.assert_array_equal(got[l][i], want[l][i], err_msg=f'learner {l}: {name}')
    assert not np.array_equal(want[l][0], before[l][0]) and not np.array_equal(want[l][1], before[l][1]) and int(want[l][3][0]) == 2, 'two steps moved the actor and its moments'
    assert all(np.array_equal(want[l][i], before[l][i]) for i in (5, 6, 7, 8)), 'a BC step moves the actor alone'
    parts = want[l][4]
    assert np.all(parts[:GUARD] == SENTINEL) and np.all(parts[GUARD + B // 16:] == SENTINEL) and np.all(parts[GUARD:GUARD + B // 16] != SENTINEL)
  for l in range(1, L):
    assert not np.array_equal(want[0][0], want[l][0]) and not np.array_equal(want[0][4], want[l][4]), 'the learners are meant to differ'
  # without the partials
  _lib.check(L_.il_bc_step_population(_lib.ptr(d_dev), _lib.ptr(b_dev), L, C.byref(pop[0].sac), None, 0, _lib.stream_ptr()))
  torch.cuda.synchronize()
  assert all(int(x.ao.step_count[0]) == 3 for x in pop) and all(np.array_equal(N(x.loss), got[l][4]) for l, x in enumerate(pop))


def test_bc_step_population_refusals():
  """IL_FLAG_GRADS_ONLY, a batch of 24, hidden 320, a short workspace and null arrays: refused by name, nothing launched (actor, moments, step count and loss partials
  keep their bytes), and the same arrays are then served by a valid call."""
  shape = (11, 3, 64, 32, 2)
  S, A, H, B, L = shape
  L_ = _lib.lib()
  pop = _bc_learners(shape)
  before = _bc_state(pop)
  d_dev, b_dev = il_training._device_array([x.sac for x in pop], DEV), il_training._device_array([x.eb for x in pop], DEV)
  loss_ptrs = torch.tensor([x.loss[GUARD:].data_ptr() for x in pop], dtype=torch.int64, device=DEV)
  dd, bb, ll, ok = _lib.ptr(d_dev), _lib.ptr(b_dev), _lib.ptr(loss_ptrs), C.byref(pop[0].sac)
  def shaped(**kw):
    d = _lib.Sac.from_buffer_copy(pop[0].sac)
    for k, v in kw.items(): setattr(d, k, v)
    return C.byref(d)
  IL_FLAG_GRADS_ONLY = 1
  for args, code, word in (((dd, bb, L, ok, ll, IL_FLAG_GRADS_ONLY), IL_ERR_ARG, b'IL_FLAG_GRADS_ONLY'), ((dd, bb, L, shaped(batch=24), ll, 0), IL_ERR_ARG, b'batch=24'),
                           ((dd, bb, L, shaped(hidden=320), ll, 0), IL_ERR_ARG, b'hidden=320'), ((dd, bb, L, shaped(action_dim=9), ll, 0), IL_ERR_ARG, b'action_dim=9'),
                           ((dd, bb, L, shaped(workspace_floats=100), ll, 0), IL_ERR_WORKSPACE, b'workspace too small (100 <'),
                           ((None, bb, L, ok, ll, 0), IL_ERR_ARG, b'null device array'), ((dd, None, L, ok, ll, 0), IL_ERR_ARG, b'null device array'),
                           ((dd, bb, L, None, ll, 0), IL_ERR_ARG, b'null shape'), ((dd, bb, 0, ok, ll, 0), IL_ERR_ARG, b'n_learners=0'), ((dd, bb, 65536, ok, ll, 0), IL_ERR_ARG, b'n_learners=65536')):
    assert L_.il_bc_step_population(*args, _lib.stream_ptr()) == code, word
    assert b'il_bc_step_population' in L_.il_last_error() and word in L_.il_last_error(), (word, L_.il_last_error())
  after = _bc_state(pop)
  assert all(np.array_equal(a, b) for la, lb in zip(before, after) for a, b in zip(la, lb)), 'a refused call launched its kernels'
  _lib.check(L_.il_bc_step_population(dd, bb, L, ok, ll, 0, _lib.stream_ptr()))
  ref = _bc_learners(shape)
  for x in ref:
    od = x.ao.desc()
    _lib.check(L_.il_bc_step(_lib.ptr(x.actor.flat), _lib.ptr(x.ao.grad), C.byref(od), S, A, H, C.byref(x.eb), C.c_void_p(x.sac.workspace), x.sac.workspace_floats, _lib.ptr(x.loss[GUARD:]), 0, _lib.stream_ptr()))
  for a, b in zip(_bc_state(pop), _bc_state(ref)):
    for x, y in zip(a, b): np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------------------------------------
# il.BatchedPopulationPlan('DRIL') against plan.run() per learner
# ---------------------------------------------------------------------------------------------
def _dril_learners(n, bc_aux, B=64, hidden=64, ensemble=None):
  """n independent DRIL learners at hopper dims (own networks, rings, index streams, Philox keys and counters, ensembles and thresholds) as UpdatePlans, reproducibly."""
  il_training._NOISE.clear(); il_training._WS.clear()
  plans, state = [], []
  S, A = gi.DIMS['hopper']
  mcfg = ensemble or Cfg(hidden_size=64, depth=1, activation='tanh', input_dropout=0.1, dropout=0.1)
  aux = bc_aux if isinstance(bc_aux, (list, tuple)) else [bc_aux] * n
  for l in range(n):
    torch.manual_seed(40 + l)   # the process seed while this learner is built: its ensemble's Philox key
    cfg = Cfg(hidden_size=hidden, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(40 + l)
    agent, expert = gi.transitions(rs, 1500, S, A), gi.transitions(rs, 600, S, A, state_shift=0.5)
    agent['actions'], expert['actions'] = (0.8 * agent['actions']).astype(np.float32), (0.8 * expert['actions']).astype(np.float32)
    mem = il.ReplayMemory(4000, S, A, True, device=DEV); fill_memory(mem, agent, 1500)
    emem = il.ReplayMemory(600, S, A, True, device=DEV); fill_memory(emem, expert, 600)
    mem.index_rng = emem.index_rng = il.IndexStream(100 + l)
    disc = il.DropoutSoftActor(S, A, mcfg, device=DEV)
    disc.flat.mul_(0.3)   # (a small head: exp(log_prob) well inside float32)
    disc.set_uncertainty_threshold(emem['states'][:600], emem['actions'][:600], 0.5)   # the median of its own expert uncertainties: both reward signs occur
    plans.append(il.UpdatePlan('DRIL', actor, critic, log_alpha, target, mem, ao, co, to, B, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=disc,
                               discriminator_optimiser=il.AdamW(disc, lr=3e-5, weight_decay=0), overlap=False, learner_id=l, bc_aux=aux[l]))
    state.append((actor, critic, target, log_alpha, ao, co, to, mem, disc))
  return plans, state


def _dril_state(plans, state):
  torch.cuda.synchronize()
  out = []
  for l, ((actor, critic, target, log_alpha, ao, co, to, mem, disc), p) in enumerate(zip(state, plans)):
    counter = il_training._noise_counter(actor.flat.device, l)   # the learner's update counter (learner_id = l): what its SAC descriptor and its ensemble's descriptor point at
    out.append([N(actor.flat), N(critic.flat), N(target.flat), N(log_alpha)] + [N(t) for o in (ao, co, to) for t in (o.exp_avg, o.exp_avg_sq, o.step_count[:1])]
               + [N(p.rewards), N(p.logp), N(p.q), N(p.idx), N(p.eidx), N(mem.stream().device_state(DEV)), N(counter), N(disc.flat)])
  return out


def _assert_same_dril_learners(a, b, updates):
  for l, (a_l, b_l) in enumerate(zip(a, b)):
    for i, (x, y) in enumerate(zip(a_l, b_l)):
      assert np.isfinite(x.astype(np.float64)).all()
      np.testing.assert_array_equal(x, y, err_msg=f'learner {l}, tensor {i}')
    assert int(a_l[19][0]) == updates, 'one bump of the noise counter per update'
    assert set(np.unique(a_l[13]).tolist()) == {-1.0, 1.0}, 'both reward signs occur'
  assert not np.array_equal(a[0][0], a[1][0]) and not np.array_equal(a[0][13], a[1][13]), 'the learners are meant to differ'


@pytest.mark.parametrize('bc_aux', [True, False], ids=['bc_aux', 'no-bc_aux'])
@pytest.mark.parametrize('how', ['overlap', 'in stream order', 'captured'])
def test_dril_population_plan_equals_plan_run_per_learner(monkeypatch, how, bc_aux):
  """Three updates of three DRIL learners: BatchedPopulationPlan (the reward launch on the side stream beside the BC auxiliary launch and the forward-only SAC launches;
  IL_POP_OVERLAP=0: in stream order; one eager run, capture(), two replays) against plan.run() per learner - actor, critic, target, log_alpha, the optimisers' moments and
  step counts, rewards, logp, q, the drawn indices, the index-stream state, the noise counter and the (untouched) ensemble, bit for bit. With bc_aux the actor optimiser
  has stepped twice per update."""
  monkeypatch.setenv('IL_POP_OVERLAP', '0' if how == 'in stream order' else '1')
  plans, state = _dril_learners(3, bc_aux)
  for _ in range(3):
    for p in plans: p.run()
  want = _dril_state(plans, state)
  plans, state = _dril_learners(3, bc_aux)
  pop = il.BatchedPopulationPlan(plans)
  assert pop.algorithm == 'DRIL' and pop.bc_aux == bc_aux and (pop.side is None) == (how == 'in stream order')
  if how == 'captured':
    pop.run()
    torch.cuda.synchronize()
    pop.capture()
    for _ in range(2): pop.replay()
  else:
    for _ in range(3): pop.run()
  got = _dril_state(plans, state)
  _assert_same_dril_learners(want, got, 3)
  assert all(int(l[6][0]) == (6 if bc_aux else 3) and int(l[9][0]) == 3 for l in got), 'actor optimiser steps: the BC auxiliary step and the SAC actor step per update'


def test_dril_population_plan_refusals():
  """Ensembles of different shapes or dropout probabilities, a learner without its threshold and a population in which only some learners have bc_aux are refused."""
  plans, _ = _dril_learners(2, True)
  plans[1].dril.hidden = 48
  with pytest.raises(AssertionError, match='share dims'):
    il.BatchedPopulationPlan(plans)
  plans, _ = _dril_learners(2, True)
  plans[1].dril.p = 0.2
  with pytest.raises(AssertionError, match='share dims'):
    il.BatchedPopulationPlan(plans)
  plans, _ = _dril_learners(2, False)
  plans[0].discriminator.q = None
  with pytest.raises(AssertionError, match='set_uncertainty_threshold'):
    il.BatchedPopulationPlan(plans)
  plans, _ = _dril_learners(2, [True, False])
  with pytest.raises(AssertionError, match='every learner of a population or for none'):
    il.BatchedPopulationPlan(plans)
  sub = il.BatchedPopulationPlan(_dril_learners(4, True)[0], groups=2)   # sub-populations are branches of one graph: no nested fork
  assert [s.side for s in sub.subs] == [None, None] and sub.algorithm == 'DRIL' and all(s.bc_aux for s in sub.subs)


# ---------------------------------------------------------------------------------------------
# train.py -m seed=... algorithm=DRIL: population schedule against per_learner
# ---------------------------------------------------------------------------------------------
from test_train_gpu import COMMON  # noqa: E402  (steps 260, batch 64, two evaluations of two episodes, 60-step episodes)

DRIL_25_DISCRIMINATOR = ['imitation.discriminator.hidden_size=32', 'imitation.discriminator.depth=2', 'imitation.discriminator.activation=relu',
                         'imitation.discriminator.input_dropout=0.4033187050372362', 'imitation.discriminator.dropout=0.556490308791399']   # the shape of conf/optimised_hyperparameters/DRIL_25_trajectories
SWEEP_CASES = [pytest.param([], id='shipped-bc_aux'), pytest.param(['imitation.bc_aux_loss=false'], id='no-bc_aux'), pytest.param(DRIL_25_DISCRIMINATOR, id='DRIL_25-ensemble'),
               pytest.param(['imitation.mix_expert_data=prefill_memory', '+acting.schedule=fused'], id='prefill-fused')]


def dril_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, short, tp, min_updates=2, iterations=50):
  """test_population_red_gpu.red_sweep_schedules_leave_the_same_bytes for DRIL (`tp`: tests/test_population_acting_gpu.py): `-m seed=3,4` under +sweep.schedule=population
  and per_learner - the same bytes in agent.pth, discriminator.pth and metrics.pth (timing keys aside), different jobs, one population."""
  argv = ['-m', 'seed=3,4', 'algorithm=DRIL', 'env=hopper', f'imitation.pretraining.iterations={iterations}'] + extra + short
  roots = {}
  for schedule in ('population', 'per_learner'):
    capsys.readouterr()
    roots[schedule], scores = tp._sweep(tmp_path, schedule, argv + [f'+sweep.schedule={schedule}'])
    err = capsys.readouterr().err
    assert err.count('[train] sweep:') == 1 and 'one population of 2 learners' in err and f'+sweep.schedule={schedule}' in err, err
    assert np.isfinite(scores).all()
    roots[schedule + ' scores'] = scores
  assert roots['population scores'] == roots['per_learner scores']
  assert os.path.basename(os.path.dirname(roots['population'])) == 'DRIL_hopper_sweeper'
  jobs = []
  for j in (0, 1):
    fp, fl = tp._job_files(roots['population'], j), tp._job_files(roots['per_learner'], j)
    assert set(fp) == set(fl) == {'agent.pth', 'discriminator.pth', 'metrics.pth'}
    for f in fp:
      a, b = fp[f], fl[f]
      if f == 'metrics.pth':
        a, b = ({k: v for k, v in m.items() if k not in tp.TIMING_KEYS} for m in (a, b))
        assert len(a['update_steps']) >= min_updates and len(a['test_steps']) == 2 and all(np.isfinite(q).all() for q in a['Q_values'])
        assert all(set(np.unique(r).tolist()) <= {-1.0, 1.0} for r in a['predicted_rewards']), 'DRIL rewards are +-1'
      tp._assert_same_nested(a, b, f'job {j}: {f}')
    assert all(torch.isfinite(v).all() for v in fp['agent.pth']['actor'].values())
    assert all(k.startswith('actor.') for k in fp['discriminator.pth']) and all(torch.isfinite(v).all() for v in fp['discriminator.pth'].values())
    jobs.append(fp)
  assert any(not torch.equal(v, jobs[1]['agent.pth']['actor'][k]) for k, v in jobs[0]['agent.pth']['actor'].items()), 'the jobs of a seed sweep are meant to differ'
  assert any(not torch.equal(v, jobs[1]['discriminator.pth'][k]) for k, v in jobs[0]['discriminator.pth'].items())
  assert jobs[0]['metrics.pth']['test_returns'] != jobs[1]['metrics.pth']['test_returns']


@pytest.mark.parametrize('extra', SWEEP_CASES)
def test_dril_seed_sweep_population_equals_per_learner(tmp_path, capsys, extra):
  import test_population_acting_gpu as tp
  dril_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, COMMON, tp)
