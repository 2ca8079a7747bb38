"""`-m gpu`: seed sweeps of GMMIL as one population. The reward launch (`il_gmmil_reward_population`: k_gmmil_mfma_pop, csrc/gmmil.hip) against one `il_gmmil_reward` per
learner, bit for bit, twice (the arrival counters of every learner's workspace reset themselves); its refusals; `il.BatchedPopulationPlan('GMMIL')` against `plan.run()`
per learner; and `python train.py -m seed=... algorithm=GMMIL` under both sweep schedules, which must leave the same bytes. The bodies also run on the host emulation of
the kernels (tests/test_population_gmmil_emulated.py)."""
import ctypes as C
import os
import subprocess
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
  from imitation_learning_amd import training as il_training
  from gpu_util import DEV, N, T, Cfg, fill_memory

GUARD, SENTINEL = 32, -7.5   # guard floats on both sides of every learner's reward buffer
IL_ERR_ARG, IL_ERR_UNSUPPORTED, IL_ERR_WORKSPACE = 1, 2, 4

# (L, n1, n2, S, A, state_only): the smallest shapes that reach each path of the kernel and of the (block, learner) grid
SHIPPED = (3, 128, 128, 18, 6, 0)        # HalfCheetah at the shipped batch: D = 24, NKQ = 2, 32-column blocks, two row blocks, 16 workgroups per learner
SHIPPED_STATE_ONLY = (3, 128, 128, 18, 6, 1)   # the state-only path: D = 18, the actions never read
HOPPER = (3, 128, 128, 12, 3, 0)         # D = 15: element loads (A = 3 is no whole lane)
RAGGED = (2, 63, 257, 11, 3, 0)          # rows and columns beyond the batch in the last row block / column block
NKQ4_EDGE = (2, 64, 64, 56, 8, 0)        # D = 64: the last width of NKQ = 4, whole 16-byte lanes
ANT = (2, 129, 127, 112, 8, 0)           # D = 120, NKQ = 8, whole lanes, one row past two row blocks
LIMIT = (2, 33, 31, 120, 8, 0)           # D = 128: the limit of the centred-Gram form
NINE_LEARNERS = (9, 16, 16, 8, 8, 0)     # more learners than the eight XCDs, two workgroups each (one row block x (1 + 1) column blocks)
KERNEL_CASES = [pytest.param(SHIPPED, id='shipped'), pytest.param(HOPPER, id='hopper-element-loads'), pytest.param(RAGGED, id='ragged'), pytest.param(NKQ4_EDGE, id='D64'),
                pytest.param(ANT, id='ant-D120'), pytest.param(LIMIT, id='D128'), pytest.param(NINE_LEARNERS, id='nine-learners'), pytest.param(SHIPPED_STATE_ONLY, id='shipped-state-only')]


def _gmmil_population(case, seed=0):
  """L learners of one shape, each with its own random policy and expert batch (its own offset and spread), its own weights - some rows with weight 0, as absorbing rows
  have -, its own bandwidths (the float64 medians of ITS data, rounded to float32), workspace and guarded output. Returns a list of dicts."""
  L, n1, n2, S, A, state_only = case
  D = S if state_only else S + A
  wsf = int(_lib.lib().il_gmmil_workspace_floats(n1, n2, D))
  out = []
  for l in range(L):
    rs = np.random.RandomState(4321 + 17 * l + seed)
    X = (rs.standard_normal((n1, S + A)) * (1.0 + 0.25 * l) + 0.3 * l).astype(np.float32)
    E = (rs.standard_normal((n2, S + A)) * 0.8 + 0.5 - 0.2 * l).astype(np.float32)
    w, we = rs.uniform(0.5, 1.5, n1).astype(np.float32), rs.uniform(0.5, 1.5, n2).astype(np.float32)
    w[rs.choice(n1, max(n1 // 8, 1), replace=False)] = 0; we[rs.choice(n2, max(n2 // 8, 1), replace=False)] = 0
    d64 = lambda a, b: ((a[:, None, :D].astype(np.float64) - b[None, :, :D].astype(np.float64)) ** 2).mean(2)
    g1, g2 = float(np.float32(1.0 / (np.median(d64(X, E)) + 1e-8))), float(np.float32(1.0 / (np.median(d64(E, E)) + 1e-8)))
    t = dict(xs=T(X[:, :S]), xa=T(X[:, S:]), es=T(E[:, :S]), ea=T(E[:, S:]), w=T(w), we=T(we))
    ln = dict(X=X, E=E, w=w, we=we, g1=g1, g2=g2, t=t, pb=il_training._sa_batch(t['xs'], t['xa'], t['w']), eb=il_training._sa_batch(t['es'], t['ea'], t['we']),
              ws=torch.zeros(wsf, dtype=torch.float32, device=DEV), buf=torch.full((GUARD + n1 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV))
    out.append(ln)
  return out, wsf


def _learner_array(learners):
  return il_training._device_array([_lib.GmmilLearner(ln['pb'], ln['eb'], ln['g1'], ln['g2'], ln['ws'].data_ptr(), ln['buf'][GUARD:].data_ptr()) for ln in learners], DEV)


def _per_learner_rewards(case, learners, wsf):
  """il_gmmil_reward on every learner's descriptors, with a workspace of its own."""
  L, n1, n2, S, A, state_only = case
  out = []
  for ln in learners:
    r, ws = torch.full((n1,), SENTINEL, dtype=torch.float32, device=DEV), torch.zeros(wsf, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().il_gmmil_reward(C.byref(ln['pb']), C.byref(ln['eb']), S, A, state_only, ln['g1'], ln['g2'], _lib.ptr(r), None, None, _lib.ptr(ws), wsf, _lib.stream_ptr()))
    out.append(r)
  torch.cuda.synchronize()
  return out


def _population_call(case, arr, wsf, whole_lanes):
  L, n1, n2, S, A, state_only = case
  return _lib.lib().il_gmmil_reward_population(_lib.ptr(arr), L, n1, n2, S, A, state_only, whole_lanes, wsf, _lib.stream_ptr())


def _assert_population_equals(case, learners, want, call):
  L, n1 = case[0], case[1]
  for l, ln in enumerate(learners):
    got = ln['buf'][GUARD:GUARD + n1]
    assert torch.isfinite(want[l]).all() and len(set(N(want[l]).tolist())) > n1 // 2, f'learner {l}: the reference rewards are meant to vary'
    assert np.array_equal(N(got), N(want[l])), f'call {call}, learner {l}: max |difference| {float((got - want[l]).abs().max()):.3e}'
    assert bool((ln['buf'][:GUARD] == SENTINEL).all()) and bool((ln['buf'][GUARD + n1:] == SENTINEL).all()), f'call {call}, learner {l}: a guard float was written'
  for l in range(1, L):   # the learners really differ: another learner's batches, weights or bandwidths would not pass
    assert not torch.equal(want[0], want[l])


@pytest.mark.parametrize('case', KERNEL_CASES)
def test_gmmil_reward_population_equals_il_gmmil_reward_per_learner(case):
  """One launch for L learners against L calls of il_gmmil_reward on the same descriptors: array_equal per learner, guard floats untouched - twice, with nothing reset in
  between: the second call runs on the counters the first one left. Learner 0's rewards also against float64, with the body and the bound of
  tests/test_gpu_parity.py::test_gmmil_direct_form_matches_float64_outside_the_mfma_range (1e-5 max|similarity|)."""
  L, n1, n2, S, A, state_only = case
  D = S if state_only else S + A
  learners, wsf = _gmmil_population(case)
  want = _per_learner_rewards(case, learners, wsf)
  lanes = il_training.gmmil_whole_lanes([b for ln in learners for b in (ln['pb'], ln['eb'])], S, A, state_only)
  assert lanes == int(S % 4 == 0 and (state_only or A % 4 == 0)), 'separately allocated tensors are 16-byte aligned: the promise follows the widths'
  arr = _learner_array(learners)
  for call in (1, 2):
    for ln in learners: ln['buf'][GUARD:GUARD + n1] = SENTINEL
    _lib.check(_population_call(case, arr, wsf, lanes))
    torch.cuda.synchronize()
    _assert_population_equals(case, learners, want, call)
  ln = learners[0]
  X, E = ln['X'][:, :D].astype(np.float64), ln['E'][:, :D].astype(np.float64)
  d64 = lambda a, b: ((a[:, None, :] - b[None, :, :]) ** 2).mean(2)
  dxe, dxx = d64(X, E), d64(X, X)
  wn, wen = ln['w'].astype(np.float64) / ln['w'].astype(np.float64).sum(), ln['we'].astype(np.float64) / ln['we'].astype(np.float64).sum()
  sim64 = sum(wn * (np.exp(-gm * dxe) @ wen) for gm in (ln['g1'], ln['g2'])); self64 = sum(wn * (np.exp(-gm * dxx) @ wn) for gm in (ln['g1'], ln['g2']))
  bound = 1e-5 * np.abs(sim64).max()
  err = np.abs(N(ln['buf'][GUARD:GUARD + n1]) - (sim64 - self64)).max() / bound
  print(f'gmmil population {case}: |reward| error / bound = {err:.3e}')
  assert err <= 1, err


def test_gmmil_reward_population_whole_lanes_is_a_promise_about_requests_not_values():
  """Aligned data (S = 56, A = 8) with whole_lanes = 0 and with 1: the same bits."""
  case = NKQ4_EDGE
  L, n1 = case[0], case[1]
  learners, wsf = _gmmil_population(case, seed=1)
  arr = _learner_array(learners)
  got = {}
  for lanes in (1, 0):
    for ln in learners: ln['buf'][GUARD:GUARD + n1] = SENTINEL
    _lib.check(_population_call(case, arr, wsf, lanes))
    torch.cuda.synchronize()
    got[lanes] = [N(ln['buf']).copy() for ln in learners]
  want = _per_learner_rewards(case, learners, wsf)
  for l in range(L):
    assert np.array_equal(got[0][l], got[1][l]) and np.array_equal(got[1][l][GUARD:GUARD + n1], N(want[l])), f'learner {l}'


def test_gmmil_reward_population_refusals():
  """The exact error codes, and nothing launched: the valid device array of a small population stays behind every call, so a launch that went out anyway would write its
  rewards (and leave tickets in the counters, which the valid call at the end would trip over)."""
  L_ = _lib.lib()
  case = (2, 33, 31, 11, 3, 0)
  L, n1, n2, S, A, state_only = case
  learners, wsf = _gmmil_population(case)
  arr = _learner_array(learners)
  a, st = _lib.ptr(arr), _lib.stream_ptr
  for args, code, word in (((None, L, n1, n2, S, A, 0, 0, wsf), IL_ERR_ARG, b'null'), ((a, 0, n1, n2, S, A, 0, 0, wsf), IL_ERR_ARG, b'n_learners=0'),
                           ((a, 65536, n1, n2, S, A, 0, 0, wsf), IL_ERR_ARG, b'n_learners=65536'), ((a, L, 0, n2, S, A, 0, 0, wsf), IL_ERR_ARG, b'n1=0'),
                           ((a, L, n1, 0, S, A, 0, 0, wsf), IL_ERR_ARG, b'n2=0'), ((a, L, n1, n2, S, A, 0, 0, wsf - 1), IL_ERR_WORKSPACE, b'workspace'),
                           ((a, L, n1, n2, 121, 8, 0, 0, 1 << 40), IL_ERR_UNSUPPORTED, b'dim=129'),
                           ((a, 65535, 1 << 15, 1 << 15, S, A, 0, 0, 1 << 40), IL_ERR_ARG, b'exceed a grid dimension')):
    assert L_.il_gmmil_reward_population(*args, st()) == code, (word, L_.il_last_error())
    assert b'il_gmmil_reward_population' in L_.il_last_error() and word in L_.il_last_error(), (word, L_.il_last_error())
  torch.cuda.synchronize()
  assert all(bool((ln['buf'] == SENTINEL).all()) and not bool(ln['ws'].any()) for ln in learners), 'a refused call launched its kernel'
  _lib.check(_population_call(case, arr, wsf, 0))   # ... and the same array is served once the call is valid
  torch.cuda.synchronize()
  _assert_population_equals(case, learners, _per_learner_rewards(case, learners, wsf), 1)


def mfma_off_body():
  """Runs in a child process under IL_GMMIL_MFMA=0 (the switch is read once per process): the population launch is refused with IL_ERR_UNSUPPORTED at a shape it otherwise
  serves, nothing is written, and il_gmmil_reward itself still answers (its direct forms)."""
  case = (2, 33, 31, 11, 3, 0)
  learners, wsf = _gmmil_population(case)
  arr = _learner_array(learners)
  assert _population_call(case, arr, wsf, 0) == IL_ERR_UNSUPPORTED and b'IL_GMMIL_MFMA=0' in _lib.lib().il_last_error(), _lib.lib().il_last_error()
  torch.cuda.synchronize()
  assert all(bool((ln['buf'] == SENTINEL).all()) and not bool(ln['ws'].any()) for ln in learners), 'a refused call launched its kernel'
  assert all(torch.isfinite(r).all() for r in _per_learner_rewards(case, learners, wsf))
  print('mfma-off ok')


MFMA_OFF_CHILD = 'import sys; sys.path[:0] = [{root!r}, {root!r} + "/tests", {root!r} + "/tests/golden"]; import test_population_gmmil_gpu as t; t.mfma_off_body()'


def test_gmmil_reward_population_is_unsupported_under_IL_GMMIL_MFMA_0(child=None):
  r = subprocess.run([sys.executable, '-c', (child or MFMA_OFF_CHILD).format(root=ROOT)], env=dict(os.environ, IL_GMMIL_MFMA='0'), cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0 and 'mfma-off ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---------------------------------------------------------------------------------------------
# il.BatchedPopulationPlan('GMMIL') against plan.run() per learner
# ---------------------------------------------------------------------------------------------
def _gmmil_learners(n, B=64, hidden=64, state_only=False, mix_expert=False):
  """n independent GMMIL learners at HalfCheetah dims (own networks, rings, index streams, Philox counters and - once their first batch has been seen - bandwidths) as
  UpdatePlans, reproducibly."""
  il_training._NOISE.clear(); il_training._WS.clear()
  plans, state = [], []
  S, A = gi.DIMS['halfcheetah']
  for l in range(n):
    torch.manual_seed(40 + l)
    cfg = Cfg(hidden_size=hidden, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(40 + l)
    mem = il.ReplayMemory(4000, S, A, True, device=DEV); fill_memory(mem, gi.transitions(rs, 1500, S, A), 1500)
    emem = il.ReplayMemory(600, S, A, True, device=DEV); fill_memory(emem, gi.transitions(rs, 600, S, A, state_shift=0.5 + 0.2 * l), 600)
    mem.index_rng = emem.index_rng = il.IndexStream(100 + l)
    disc = il.GMMILDiscriminator(S, A, Cfg(state_only=state_only))
    plans.append(il.UpdatePlan('GMMIL', actor, critic, log_alpha, target, mem, ao, co, to, B, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=disc, overlap=False, learner_id=l,
                               mix_expert=mix_expert))
    state.append((actor, critic, target, log_alpha, ao, co, to, mem))
  return plans, state


def _gmmil_state(plans, state):
  torch.cuda.synchronize()
  out = []
  for (actor, critic, target, log_alpha, ao, co, to, mem), p in zip(state, plans):
    out.append([N(actor.flat), N(critic.flat), N(target.flat), N(log_alpha)] + [N(t) for o in (ao, co, to) for t in (o.exp_avg, o.exp_avg_sq, o.step_count[:1])]
               + [N(p.rewards), N(p.logp), N(p.q), N(p.idx), N(p.eidx), N(mem.stream().device_state(DEV)), np.array([p.discriminator.gamma_1, p.discriminator.gamma_2], np.float64)])
  return out


def _assert_same_learners(a, b):
  for l, (a_l, b_l) in enumerate(zip(a, b)):
    for i, (x, y) in enumerate(zip(a_l, b_l)):
      assert np.isfinite(x.astype(np.float64)).all()
      np.testing.assert_array_equal(x, y, err_msg=f'learner {l}, tensor {i}')
  assert not np.array_equal(a[0][0], a[1][0]) and not np.array_equal(a[0][13], a[1][13]) and not np.array_equal(a[0][19], a[1][19]), 'the learners are meant to differ'


@pytest.mark.parametrize('how', ['overlap', 'in stream order', 'captured'])
def test_gmmil_population_plan_equals_plan_run_per_learner(monkeypatch, how):
  """Four updates of three GMMIL learners: BatchedPopulationPlan - the first run() eager (every learner's bandwidths from its own first batch), then the reward launch beside
  the forward-only SAC launches on the side stream; IL_POP_OVERLAP=0: in stream order; captured: capture() after the first run, three replays - against plan.run() per
  learner: actor, critic, target, log_alpha, the optimisers' moments and step counts, rewards, logp, q, the drawn indices, the index-stream state and the frozen
  bandwidths, bit for bit. A capture in front of the first run is refused."""
  monkeypatch.setenv('IL_POP_OVERLAP', '0' if how == 'in stream order' else '1')
  plans, state = _gmmil_learners(3)
  for _ in range(4):
    for p in plans: p.run()
  want = _gmmil_state(plans, state)
  plans, state = _gmmil_learners(3)
  pop = il.BatchedPopulationPlan(plans)
  assert pop.algorithm == 'GMMIL' and (pop.side is None) == (how == 'in stream order')
  if how == 'captured':
    with pytest.raises(AssertionError, match=r'UpdatePlan\(GMMIL\): run\(\) once before capture\(\)'):
      pop.capture()
    assert all(p.discriminator.gamma_1 is None for p in plans) and pop.graph is None
    pop.run()
    torch.cuda.synchronize()
    pop.capture()
    for _ in range(3): pop.replay()
  else:
    for _ in range(4): pop.run()
  assert pop.gmmil_learners is not None and pop.gmmil_ws.shape[0] == 3
  _assert_same_learners(want, _gmmil_state(plans, state))


def test_gmmil_population_plan_refuses_mismatched_learners():
  plans = _gmmil_learners(1, B=64)[0] + _gmmil_learners(1, B=32)[0]
  with pytest.raises(AssertionError, match='one batch size'):
    il.BatchedPopulationPlan(plans)
  plans = _gmmil_learners(1)[0] + _gmmil_learners(1, state_only=True)[0]
  with pytest.raises(AssertionError, match='share state_size, action_size and state_only'):
    il.BatchedPopulationPlan(plans)
  with pytest.raises(AssertionError, match='mixed batches'):
    il.BatchedPopulationPlan(_gmmil_learners(2, mix_expert=True)[0])
  sub = il.BatchedPopulationPlan(_gmmil_learners(4)[0], groups=2)   # sub-populations are branches of one graph: no nested fork
  assert [s.side for s in sub.subs] == [None, None] and sub.algorithm == 'GMMIL'


# ---------------------------------------------------------------------------------------------
# train.py -m seed=... algorithm=GMMIL: population schedule against per_learner
# ---------------------------------------------------------------------------------------------
from test_train_gpu import COMMON  # noqa: E402  (steps 260, batch 64, two evaluations of two episodes, 60-step episodes)

SWEEP_CASES = [pytest.param([], id='shipped'),
               pytest.param(['optimised_hyperparameters=GMMIL_25_trajectories', 'training.batch_size=128'], id='GMMIL_25-batch128'),   # (COMMON's own batch_size would override the overlay's)
               pytest.param(['imitation.mix_expert_data=prefill_memory'], id='prefill_memory')]


def gmmil_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, short, tp, min_updates=2):
  """test_population_acting_gpu.sweep_schedules_leave_the_same_bytes for GMMIL (`tp`: that module): `-m seed=3,4` under +sweep.schedule=population and per_learner - the
  same bytes in agent.pth and metrics.pth (timing keys aside) and, as after train(), no discriminator.pth; different jobs; one population, no fallback line."""
  argv = ['-m', 'seed=3,4', 'algorithm=GMMIL', 'env=hopper'] + short + extra
  roots = {}
  for schedule in ('population', 'per_learner'):
    capsys.readouterr()
    roots[schedule], scores = tp._sweep(tmp_path, schedule, argv + [f'+sweep.schedule={schedule}'])
    err = capsys.readouterr().err
    assert err.count('[train] sweep:') == 1 and 'one population of 2 learners' in err and f'+sweep.schedule={schedule}' in err and 'one job after another' not in err, err
    assert np.isfinite(scores).all()
    roots[schedule + ' scores'] = scores
  assert roots['population scores'] == roots['per_learner scores']
  assert os.path.basename(os.path.dirname(roots['population'])) == 'GMMIL_hopper_sweeper'
  jobs = []
  for j in (0, 1):
    fp, fl = tp._job_files(roots['population'], j), tp._job_files(roots['per_learner'], j)
    assert set(fp) == set(fl) == {'agent.pth', 'metrics.pth'}
    for f in fp:
      a, b = fp[f], fl[f]
      if f == 'metrics.pth':
        a, b = ({k: v for k, v in m.items() if k not in tp.TIMING_KEYS} for m in (a, b))
        assert len(a['update_steps']) >= min_updates and len(a['test_steps']) == 2 and all(np.isfinite(q).all() for q in a['Q_values'])
        assert all(np.isfinite(r).all() and r.shape == a['predicted_rewards'][0].shape for r in a['predicted_rewards'])
      tp._assert_same_nested(a, b, f'job {j}: {f}')
    assert all(torch.isfinite(v).all() for v in fp['agent.pth']['actor'].values())
    jobs.append(fp)
  assert any(not torch.equal(v, jobs[1]['agent.pth']['actor'][k]) for k, v in jobs[0]['agent.pth']['actor'].items()), 'the jobs of a seed sweep are meant to differ'
  assert jobs[0]['metrics.pth']['test_returns'] != jobs[1]['metrics.pth']['test_returns']
  return jobs


@pytest.mark.parametrize('extra', SWEEP_CASES)
def test_gmmil_seed_sweep_population_equals_per_learner(tmp_path, capsys, extra):
  import test_population_acting_gpu as tp
  jobs = gmmil_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, COMMON, tp)
  if 'training.batch_size=128' in extra:
    assert jobs[0]['metrics.pth']['predicted_rewards'][0].shape == (128,)
