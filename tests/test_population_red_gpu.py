"""`-m gpu`: seed sweeps of RED as one population. The reward launch (`il_red_reward_population`: k_red_eval_population, csrc/red.hip) against one `il_red_forward(training = 0)`
per learner, bit for bit; its refusals; `il.BatchedPopulationPlan('RED')` against `plan.run()` per learner; and `python train.py -m seed=... algorithm=RED` under both sweep
schedules, which must leave the same bytes. The bodies also run on the host emulation of the kernels (tests/test_population_red_emulated.py)."""
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

GUARD, SENTINEL = 32, -7.5   # guard floats on both sides of every learner's reward buffer

# (S, A, H, depth, activation, state_only, B, L, p_in, p)
SHIPPED = (11, 3, 32, 1, 'relu', 0, 64, 3, 0.0, 0.0)        # conf/algorithm/RED.yaml's discriminator
RED_25 = (17, 6, 64, 2, 'tanh', 0, 48, 2, 0.05, 0.4)        # RED_25_trajectories' shape: 48 rows leave the second 32-row tile half empty; dropout set, and must not apply
STATE_ONLY = (11, 3, 32, 1, 'relu', 1, 16, 1, 0.0, 0.0)     # state_only, odd input width 11, one learner, less than one tile
LIMIT = (120, 8, 256, 1, 'relu', 0, 32, 2, 0.0, 0.0)        # the limit width: 148736 bytes of LDS, the > 64 KiB opt-in of the new kernel
KERNEL_CASES = [pytest.param(SHIPPED, id='shipped'), pytest.param(RED_25, id='RED_25-tanh-depth2-dropout'), pytest.param(STATE_ONLY, id='state_only-one-learner'),
                pytest.param(LIMIT, id='limit-width')]


def _red_population(case, seed=0):
  """L discriminators of one shape in eval mode - own random predictor and target, own batch, own sigma_1 (a factor 10 apart) - as (descriptors, batch descriptors, keep)."""
  S, A, H, depth, activation, state_only, B, L, p_in, p = case
  icfg = Cfg(state_only=bool(state_only), reward_bandwidth_scale=None, discriminator=Cfg(hidden_size=H, depth=depth, activation=activation, input_dropout=p_in, dropout=p))
  rs = np.random.RandomState(1234 + seed)
  D = S if state_only else S + A
  descs, batches, keep = [], [], []
  for l in range(L):
    d = il.REDDiscriminator(S, A, icfg, device=DEV)
    lay = [(H, D)] + [(H, H)] * (depth - 1) + [(D, H)]
    for flat in (d.flat, d.target_flat):   # torch order: W [out, in] then b, per layer; fan-in scaling keeps the embeddings O(1)
      flat.copy_(T(np.concatenate([np.concatenate([(rs.standard_normal(o * i) / np.sqrt(i)).astype(np.float32), (0.1 * rs.standard_normal(o)).astype(np.float32)]) for o, i in lay])))
    d.sigma_1 = 0.05 * 10.0 ** l
    d.eval()
    tr = {k: T(v) for k, v in gi.transitions(rs, B, S, A).items() if k in ('states', 'actions', 'rewards', 'next_states', 'terminals', 'weights', 'absorbing')}
    desc, b = d._desc(B), il.memory.batch_desc(tr)
    assert (desc.p_in, desc.p) == (np.float32(p_in), np.float32(p)) and desc.sigma_1 == np.float32(d.sigma_1)
    descs.append(desc); batches.append(b); keep.append((d, tr))
  return descs, batches, keep


def _guarded(L, B):
  bufs = [torch.full((GUARD + B + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(L)]
  ptrs = torch.tensor([b[GUARD:].data_ptr() for b in bufs], dtype=torch.int64, device=DEV)
  return bufs, ptrs


def _per_learner_rewards(descs, batches, B, training=0):
  out = []
  for desc, b in zip(descs, batches):
    r = torch.full((B,), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().il_red_forward(C.byref(desc), C.byref(b), training, None, None, None, 7, _lib.ptr(r), None, None, _lib.stream_ptr()))
    out.append(r)
  torch.cuda.synchronize()
  return out


@pytest.mark.parametrize('case', KERNEL_CASES)
def test_red_reward_population_equals_il_red_forward_per_learner(case):
  """One launch for L learners against L calls of il_red_forward(training = 0): torch.equal per learner, guard floats untouched. The host descriptor is learner 0's, so a
  kernel that took the bandwidth (or the parameters) from it instead of from the learner's device descriptor fails for every other learner."""
  S, A, H, depth, activation, state_only, B, L, p_in, p = case
  descs, batches, keep = _red_population(case)
  want = _per_learner_rewards(descs, batches, B)
  bufs, ptrs = _guarded(L, B)
  d_dev, b_dev = il_training._device_array(descs, DEV), il_training._device_array(batches, DEV)
  _lib.check(_lib.lib().il_red_reward_population(_lib.ptr(d_dev), _lib.ptr(b_dev), _lib.ptr(ptrs), L, C.byref(descs[0]), _lib.stream_ptr()))
  torch.cuda.synchronize()
  for l in range(L):
    got = bufs[l][GUARD:GUARD + B]
    assert torch.isfinite(want[l]).all() and float(want[l].min()) >= 0.0 and float(want[l].max()) <= 1.0 and len(set(N(want[l]).tolist())) > B // 2, f'learner {l}: the reference rewards are meant to vary'
    assert torch.equal(got, want[l]), f'learner {l}: max |difference| {float((got - want[l]).abs().max()):.3e}'
    assert bool((bufs[l][:GUARD] == SENTINEL).all()) and bool((bufs[l][GUARD + B:] == SENTINEL).all()), f'learner {l}: a guard float was written'
  for l in range(1, L):   # the learners really differ: another learner's parameters, batch or bandwidth would not pass
    assert not torch.equal(want[0], want[l])
    wrong_sigma = torch.exp(torch.log(want[l].double()) * (descs[0].sigma_1 / descs[l].sigma_1)).float()   # learner l's rewards under learner 0's bandwidth
    assert not torch.allclose(wrong_sigma, want[l], rtol=1e-3, atol=0)
  if p > 0:   # the descriptors carry dropout: train mode would give other values, so equality with training = 0 shows that none was applied
    dropped = _per_learner_rewards(descs, batches, B, training=1)
    assert all(not torch.equal(a, b) for a, b in zip(dropped, want))


def _bare_shape(S, A, H, depth, activation, B, some):
  d = _lib.Red()
  d.state_dim, d.action_dim, d.hidden, d.batch, d.state_only, d.depth, d.activation = S, A, H, B, 0, depth, activation
  d.predictor = d.target = some.data_ptr()
  return d


def test_red_reward_population_refusals():
  """Every refusal names the entry point or the limit, and nothing is launched: the valid device arrays of a one-learner population stay behind every call, so a launch
  that went out anyway would write its rewards."""
  L_ = _lib.lib()
  S, A, H, depth, activation, state_only, B, L, p_in, p = STATE_ONLY
  descs, batches, keep = _red_population(STATE_ONLY)
  bufs, ptrs = _guarded(L, B)
  d_dev, b_dev = il_training._device_array(descs, DEV), il_training._device_array(batches, DEV)
  dd, bb, pp, ok = _lib.ptr(d_dev), _lib.ptr(b_dev), _lib.ptr(ptrs), C.byref(descs[0])
  some = torch.zeros(64, dtype=torch.float32, device=DEV)
  IL_ERR_ARG, IL_ERR_UNSUPPORTED = 1, 2
  too_big = _bare_shape(120, 8, 256, 2, 0, B, some)     # depth 2 at input 128 / hidden 256: 247424 bytes of LDS
  assert L_.il_red_reward_population(dd, bb, pp, L, C.byref(too_big), _lib.stream_ptr()) == IL_ERR_UNSUPPORTED
  assert b'LDS' in L_.il_last_error() and b'160 KiB' in L_.il_last_error(), L_.il_last_error()
  for args, word in (((None, bb, pp, L, ok), b'null device array'), ((dd, None, pp, L, ok), b'null device array'), ((dd, bb, None, L, ok), b'null device array'),
                     ((dd, bb, pp, L, None), b'null shape'), ((dd, bb, pp, 0, ok), b'n_learners=0'), ((dd, bb, pp, 65536, ok), b'n_learners=65536'),
                     ((dd, bb, pp, L, C.byref(_bare_shape(11, 3, 257, 1, 0, B, some))), b'hidden=257'), ((dd, bb, pp, L, C.byref(_bare_shape(11, 3, 32, 1, 2, B, some))), b'activation'),
                     ((dd, bb, pp, L, C.byref(_bare_shape(121, 8, 32, 1, 0, B, some))), b'input=129'), ((dd, bb, pp, L, C.byref(_bare_shape(11, 3, 32, 3, 0, B, some))), b'depth')):
    assert L_.il_red_reward_population(*args, _lib.stream_ptr()) == IL_ERR_ARG, word
    assert b'il_red' in L_.il_last_error() and word in L_.il_last_error(), (word, L_.il_last_error())
  torch.cuda.synchronize()
  assert all(bool((b == SENTINEL).all()) for b in bufs), 'a refused call launched its kernel'
  _lib.check(L_.il_red_reward_population(dd, bb, pp, L, ok, _lib.stream_ptr()))   # ... and the same arrays are served once the call is valid
  torch.cuda.synchronize()
  assert torch.equal(bufs[0][GUARD:GUARD + B], _per_learner_rewards(descs, batches, B)[0])


# ---------------------------------------------------------------------------------------------
# il.BatchedPopulationPlan('RED') against plan.run() per learner
# ---------------------------------------------------------------------------------------------
def _red_learners(n, B=64, hidden=64):
  """n independent RED learners at hopper dims (own networks, rings, index streams, Philox counters, discriminators and bandwidths) as UpdatePlans, reproducibly."""
  il_training._NOISE.clear(); il_training._WS.clear()
  plans, state = [], []
  S, A = gi.DIMS['hopper']
  icfg = Cfg(state_only=False, reward_bandwidth_scale=None, discriminator=Cfg(hidden_size=32, depth=1, activation='relu', input_dropout=0, dropout=0))
  for l in range(n):
    torch.manual_seed(30 + l)
    cfg = Cfg(hidden_size=hidden, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(30 + l)
    mem = il.ReplayMemory(4000, S, A, True, device=DEV); fill_memory(mem, gi.transitions(rs, 1500, S, A), 1500)
    emem = il.ReplayMemory(600, S, A, True, device=DEV); fill_memory(emem, gi.transitions(rs, 600, S, A, state_shift=0.5), 600)
    mem.index_rng = emem.index_rng = il.IndexStream(100 + l)
    disc = il.REDDiscriminator(S, A, icfg, device=DEV)
    disc.flat.add_(0.05 * torch.randn_like(disc.flat))   # (a predictor that has moved off its initialisation)
    disc.sigma_1 = 0.4 * 10.0 ** l
    disc.eval()
    plans.append(il.UpdatePlan('RED', actor, critic, log_alpha, target, mem, ao, co, to, B, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=disc,
                               discriminator_optimiser=il.AdamW(disc, lr=3e-5, weight_decay=0), overlap=False, learner_id=l))
    state.append((actor, critic, target, log_alpha, ao, co, to, mem))
  return plans, state


def _red_state(plans, state):
  torch.cuda.synchronize()
  out = []
  for (actor, critic, target, log_alpha, ao, co, to, mem), p in zip(state, plans):
    out.append([N(actor.flat), N(critic.flat), N(target.flat), N(log_alpha)] + [N(t) for o in (ao, co, to) for t in (o.exp_avg, o.exp_avg_sq, o.step_count[:1])]
               + [N(p.rewards), N(p.logp), N(p.q), N(p.idx), N(p.eidx), N(mem.stream().device_state(DEV))])
  return out


def _assert_same_learners(a, b):
  for l, (a_l, b_l) in enumerate(zip(a, b)):
    for i, (x, y) in enumerate(zip(a_l, b_l)):
      assert np.isfinite(x.astype(np.float64)).all()
      np.testing.assert_array_equal(x, y, err_msg=f'learner {l}, tensor {i}')
  assert not np.array_equal(a[0][0], a[1][0]) and not np.array_equal(a[0][13], a[1][13]), 'the learners are meant to differ'


@pytest.mark.parametrize('how', ['overlap', 'in stream order', 'captured'])
def test_red_population_plan_equals_plan_run_per_learner(monkeypatch, how):
  """Three updates of three RED learners: BatchedPopulationPlan (the reward launch beside the forward-only SAC launches on the side stream; IL_POP_OVERLAP=0: in stream
  order; one eager run, capture(), two replays) against plan.run() per learner - actor, critic, target, log_alpha, the optimisers' moments and step counts, rewards, logp,
  q, the drawn indices and the index-stream state, bit for bit."""
  monkeypatch.setenv('IL_POP_OVERLAP', '0' if how == 'in stream order' else '1')
  plans, state = _red_learners(3)
  for _ in range(3):
    for p in plans: p.run()
  want = _red_state(plans, state)
  plans, state = _red_learners(3)
  pop = il.BatchedPopulationPlan(plans)
  assert pop.algorithm == 'RED' and (pop.side is None) == (how == 'in stream order')
  if how == 'captured':
    pop.run()
    torch.cuda.synchronize()
    pop.capture()
    for _ in range(2): pop.replay()
  else:
    for _ in range(3): pop.run()
  _assert_same_learners(want, _red_state(plans, state))
  assert all(0.0 <= float(r.min()) and float(r.max()) <= 1.0 for r in (p.rewards for p in plans))


def test_red_population_plan_refuses_mismatched_discriminators():
  plans, _ = _red_learners(2)
  plans[1].red.hidden = 48
  with pytest.raises(AssertionError, match='share dims'):
    il.BatchedPopulationPlan(plans)
  sub = il.BatchedPopulationPlan(_red_learners(4)[0], groups=2)   # sub-populations are branches of one graph: no nested fork
  assert [s.side for s in sub.subs] == [None, None] and sub.algorithm == 'RED'


# ---------------------------------------------------------------------------------------------
# train.py -m seed=... algorithm=RED: population schedule against per_learner
# ---------------------------------------------------------------------------------------------
from test_train_gpu import COMMON  # noqa: E402  (steps 260, batch 64, two evaluations of two episodes, 60-step episodes)

RED_25_DISCRIMINATOR = ['imitation.discriminator.hidden_size=64', 'imitation.discriminator.depth=2', 'imitation.discriminator.activation=tanh',
                        'imitation.discriminator.input_dropout=0.05', 'imitation.discriminator.dropout=0.4']   # the shape of conf/optimised_hyperparameters/RED_25_trajectories
SWEEP_CASES = [pytest.param([], id='shipped'), pytest.param(RED_25_DISCRIMINATOR + ['imitation.mix_expert_data=prefill_memory', '+acting.schedule=fused'], id='RED_25-prefill-fused')]


def red_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, short, tp, min_updates=2):
  """test_population_acting_gpu.sweep_schedules_leave_the_same_bytes for RED (`tp`: that module), whose jobs also leave a discriminator.pth: `-m seed=3,4` under
  +sweep.schedule=population and per_learner - the same bytes in agent.pth, discriminator.pth and metrics.pth (timing keys aside), different jobs, one population."""
  argv = ['-m', 'seed=3,4', 'algorithm=RED', 'env=hopper', 'imitation.pretraining.iterations=20'] + extra + short
  roots = {}
  for schedule in ('population', 'per_learner'):
    capsys.readouterr()
    roots[schedule], scores = tp._sweep(tmp_path, schedule, argv + [f'+sweep.schedule={schedule}'])
    err = capsys.readouterr().err
    assert err.count('[train] sweep:') == 1 and 'one population of 2 learners' in err and f'+sweep.schedule={schedule}' in err, err
    assert np.isfinite(scores).all()
    roots[schedule + ' scores'] = scores
  assert roots['population scores'] == roots['per_learner scores']
  assert os.path.basename(os.path.dirname(roots['population'])) == 'RED_hopper_sweeper'
  jobs = []
  for j in (0, 1):
    fp, fl = tp._job_files(roots['population'], j), tp._job_files(roots['per_learner'], j)
    assert set(fp) == set(fl) == {'agent.pth', 'discriminator.pth', 'metrics.pth'}
    for f in fp:
      a, b = fp[f], fl[f]
      if f == 'metrics.pth':
        a, b = ({k: v for k, v in m.items() if k not in tp.TIMING_KEYS} for m in (a, b))
        assert len(a['update_steps']) >= min_updates and len(a['test_steps']) == 2 and all(np.isfinite(q).all() for q in a['Q_values'])
        assert all(0.0 <= float(np.min(r)) and float(np.max(r)) <= 1.0 for r in a['predicted_rewards']), 'RED rewards are exp(-sigma_1 * error)'
      tp._assert_same_nested(a, b, f'job {j}: {f}')
    assert all(torch.isfinite(v).all() for v in fp['agent.pth']['actor'].values())
    assert any(k.startswith('predictor.') for k in fp['discriminator.pth']) and any(k.startswith('target.') for k in fp['discriminator.pth'])
    jobs.append(fp)
  assert any(not torch.equal(v, jobs[1]['agent.pth']['actor'][k]) for k, v in jobs[0]['agent.pth']['actor'].items()), 'the jobs of a seed sweep are meant to differ'
  assert any(not torch.equal(v, jobs[1]['discriminator.pth'][k]) for k, v in jobs[0]['discriminator.pth'].items())
  assert jobs[0]['metrics.pth']['test_returns'] != jobs[1]['metrics.pth']['test_returns']


@pytest.mark.parametrize('extra', SWEEP_CASES)
def test_red_seed_sweep_population_equals_per_learner(tmp_path, capsys, extra):
  import test_population_acting_gpu as tp
  red_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, COMMON, tp)
