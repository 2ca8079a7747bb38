"""`-m gpu`: seed sweeps of AdRIL / SQIL as one population. The relabel launch (`il_batch_mix_relabel_population`: k_mix_relabel_population, csrc/replay.hip) against one
`il_batch_mix_relabel_dyn` per learner, bit for bit (the sign of the -0.0 a row of the current round gets included), and against oracle/adril.py by value; its refusals;
`il.BatchedPopulationPlan('AdRIL')` against `plan.relabel_args(...); plan.run()` per learner; and `python train.py -m seed=... algorithm=AdRIL +sweep.adril_population=true`
under both sweep schedules, which must leave the same bytes. The bodies also run on the host emulation of the kernels (tests/test_population_adril_emulated.py)."""
import os

import numpy as np
import pytest
import torch

import inputs as gi
from oracle import adril as oadril

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib
  from imitation_learning_amd import memory as il_memory
  from imitation_learning_amd import training as il_training
  from gpu_util import DEV, N, T, Cfg, fill_memory

GUARD, SENTINEL = 32, -7.5   # guard floats (a whole number of 16-byte lanes) on both sides of every learner's rows
KEY = '+sweep.adril_population=true'
DIMS = [pytest.param((11, 3), id='hopper-S11-A3'), pytest.param((18, 6), id='halfcheetah-absorbing-S18-A6'), pytest.param((40, 17), id='wide-S40-A17')]
MODES = [pytest.param((0, 0), id='label0-mix'), pytest.param((1, 0), id='label1-SQIL'), pytest.param((2, 1), id='label2-AdRIL-freq1'), pytest.param((2, 3), id='label2-AdRIL-freq3'),
         pytest.param((2, 1250), id='label2-AdRIL-freq1250')]
BATCHES = (16, 48, 272)   # one strip; not a power of two; several workgroups per learner
TRAJECTORIES = (0, 1000003, 7, 1, 12)   # policy trajectories per learner: 0 is clamped to 1


def _learner_sets(n):
  """n_expert per learner: one learner; an all-policy, an all-expert and a half-and-half learner side by side; and the clamps (n + 7 -> n, -3 -> 0) beside ragged counts."""
  return ([n // 3], [0, n, n // 2], [5, n - 1, n + 7, -3, 1])


def _bits(t):
  return t.contiguous().view(torch.int32)


def _guarded_rows(values):
  """[n, row] values between guard floats: (buffer, view of the rows inside it)."""
  n, row = values.shape
  buf = torch.full((GUARD + n * row + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
  rows = buf[GUARD:GUARD + n * row].view(n, row)
  rows.copy_(values)
  return buf, rows


def _stamps(rs, n, update_freq, round_num):
  """Step stamps around the ceil edge: exact multiples of update_freq and their successors, the last rounds' and the current round's, then random older ones."""
  f = max(update_freq, 1)
  base = (round_num - 1) * f   # the last step of the round before the current one
  edge = [base, base + 1, max(base - 1, 1), base + f, max(base - f, 1), max(base - f + 1, 1), f, f + 1, 2 * f, 2 * f + 1, 1]
  out = np.array([edge[i % len(edge)] if i % 2 == 0 else rs.randint(1, base + f + 1) for i in range(n)], dtype=np.float32)
  return out[rs.permutation(n)]


def _case(dims, mode, n, n_experts, seed):
  """One population: per learner (policy rows, expert rows, dyn words, reward_expert) on the host, reproducibly."""
  S, A = dims
  label, update_freq = mode
  row, o_rew = int(_lib.lib().il_ring_row_floats(S, A)), 2 * S + A
  rs = np.random.RandomState(seed)
  learners = []
  for l, n_expert in enumerate(n_experts):
    step = max(update_freq, 1) * (5 + l) + (l % 2)   # an exact multiple of update_freq (round 5 + l) or its successor (round 6 + l)
    round_num = -(-step // update_freq) if update_freq > 0 else 0
    pol, exp = rs.standard_normal((n, row)).astype(np.float32), (rs.standard_normal((n, row)) + 3).astype(np.float32)
    pol[:, o_rew + 4] = _stamps(rs, n, update_freq, max(round_num, 1))
    exp[:, o_rew + 4] = rs.randint(1, 5000, n).astype(np.float32)
    learners.append((pol, exp, [n_expert, round_num, TRAJECTORIES[l % len(TRAJECTORIES)]], float(np.float32(1 / (3 + l)))))
  return learners, row, o_rew


def _device_side(learners):
  out = []
  for pol, exp, dyn, reward_expert in learners:
    buf, rows = _guarded_rows(T(pol))
    out.append((buf, rows, T(exp), torch.tensor(dyn, dtype=torch.int64).to(DEV), reward_expert))
  return out


def _per_learner(learners, n, dims, mode):
  """The reference: one il_batch_mix_relabel_dyn per learner on its own copy."""
  dev = _device_side(learners)
  for buf, rows, erows, dyn, reward_expert in dev:
    _lib.check(_lib.lib().il_batch_mix_relabel_dyn(_lib.ptr(rows), _lib.ptr(erows), n, dims[0], dims[1], mode[0], mode[1], reward_expert, _lib.ptr(dyn), _lib.stream_ptr()))
  torch.cuda.synchronize()
  return dev


def _population(learners, n, dims, mode, dev=None):
  dev = dev or _device_side(learners)
  dyn = torch.stack([d[3] for d in dev]).contiguous()   # (L, 3), as the plan keeps it: learner l's words are row l
  descs = il_training._device_array([_lib.MixLearner(rows.data_ptr(), erows.data_ptr(), dyn[l].data_ptr(), reward_expert) for l, (_, rows, erows, _, reward_expert) in enumerate(dev)], DEV)
  rc = _lib.lib().il_batch_mix_relabel_population(_lib.ptr(descs), len(dev), n, dims[0], dims[1], mode[0], mode[1], _lib.stream_ptr())
  torch.cuda.synchronize()
  return rc, dev, (descs, dyn)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dims', DIMS)
def test_mix_relabel_population_equals_il_batch_mix_relabel_dyn_per_learner(dims, mode):
  """One launch for L learners against L calls of il_batch_mix_relabel_dyn: every float of every learner's rows through an int32 view (so -0.0 is not 0.0), the guard
  floats untouched, the expert rows unchanged. Learners differ in n_expert (0, n, halves, clamped from both sides), round, trajectory count (0 clamped to 1, a large one)
  and reward_expert, so a kernel that read another learner's descriptor or dyn words fails."""
  label, update_freq = mode
  current = older = 0
  for n in BATCHES:
    for s, n_experts in enumerate(_learner_sets(n)):
      learners, row, o_rew = _case(dims, mode, n, n_experts, 7 * n + s)
      want = _per_learner(learners, n, dims, mode)
      rc, got, _ = _population(learners, n, dims, mode)
      assert rc == 0, _lib.lib().il_last_error()
      for l, ((wbuf, wrows, _, _, _), (gbuf, grows, gerows, _, _)) in enumerate(zip(want, got)):
        what = f'n {n}, learner {l} of {len(n_experts)} (n_expert {n_experts[l]})'
        assert torch.equal(_bits(grows), _bits(wrows)), what
        assert bool((gbuf[:GUARD] == SENTINEL).all()) and bool((gbuf[GUARD + n * row:] == SENTINEL).all()), f'{what}: a guard float was written'
        assert torch.equal(_bits(gerows), _bits(T(learners[l][1]))), f'{what}: the expert rows changed'
        ne = min(max(n_experts[l], 0), n)
        assert torch.equal(grows[:ne, :o_rew], gerows[:ne, :o_rew]) and torch.equal(grows[ne:, :o_rew], T(learners[l][0])[ne:, :o_rew]), what   # the reference itself mixed
        if label == 2:
          r = _bits(grows[ne:, o_rew])
          current += int((r == -2 ** 31).sum()); older += int((grows[ne:, o_rew] < 0).sum())
          assert bool(((r == -2 ** 31) | (grows[ne:, o_rew] < 0)).all()), what
          if ne: assert bool((grows[:ne, o_rew] == learners[l][3]).all())
  if label == 2: assert current > 20 and older > 20, 'rows of the current round (-0.0) and older rows (-1 / trajectories) are both meant to occur'


@pytest.mark.parametrize('mode', [pytest.param((2, 1250), id='label2-AdRIL'), pytest.param((1, 0), id='label1-SQIL')])
def test_mix_relabel_population_against_the_oracle(mode):
  """Three learners - halves, a balanced expert turn, a balanced policy turn - against oracle/adril.py's restatement of models.py:293-318, every field by value."""
  S, A = 18, 6
  label, update_freq = mode
  n, step = 48, gi.ADRIL_STEP
  turns = [(False, True), (True, True), (True, False)]   # (balanced, sample_expert) per learner
  host, dev, want = [], [], []
  for l, (balanced, sample_expert) in enumerate(turns):
    pol, exp = gi.adril_batches(80 + l, n, S, A)
    views = []
    for batch in (pol, exp):
      rows = torch.zeros(n, int(_lib.lib().il_ring_row_floats(S, A)), device=DEV)
      v = il_memory.batch_views(rows, S, A, True)
      for k in il_memory.FIELDS: v[k].copy_(T(batch[k]))
      views.append((rows, v))
    orel = oadril.RelabellerOracle(update_freq, balanced)
    orel.sample_expert = sample_expert
    n_expert = orel.resample_and_relabel(pol, exp, step + l, gi.ADRIL_TRAJ + l, 5 + l)
    want.append(pol)
    dyn = [n_expert, -(-(step + l) // update_freq) if update_freq else 0, gi.ADRIL_TRAJ + l]
    dev.append((None, views[0][0], views[1][0], torch.tensor(dyn, dtype=torch.int64).to(DEV), float(np.float32(1 / (5 + l)))))
    host.append(views[0][1])
  rc, _, _ = _population(None, n, (S, A), mode, dev=dev)
  assert rc == 0, _lib.lib().il_last_error()
  for l, (views, pol) in enumerate(zip(host, want)):
    for k in il_memory.FIELDS + ('absorbing',):
      assert N(views[k]).tobytes() == np.asarray(pol[k], np.float32).tobytes(), (l, k)   # includes the sign of -0.0 rewards


def test_mix_relabel_population_serves_rows_off_the_16_byte_grid():
  """A row buffer one float off the 16-byte grid (not what the plan builds) takes the kernel's one-float lanes: the same bits, and no access beside the rows."""
  dims, mode, n = (18, 6), (2, 3), 48
  learners, row, o_rew = _case(dims, mode, n, [n // 2, n], 5)
  want = _per_learner(learners, n, dims, mode)
  dev = []
  for pol, exp, dyn, reward_expert in learners:
    buf = torch.full((GUARD + 1 + n * row + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    rows = buf[GUARD + 1:GUARD + 1 + n * row].view(n, row)
    rows.copy_(T(pol))
    assert rows.data_ptr() % 16 == 4
    dev.append((buf, rows, T(exp), torch.tensor(dyn, dtype=torch.int64).to(DEV), reward_expert))
  rc, got, _ = _population(None, n, dims, mode, dev=dev)
  assert rc == 0, _lib.lib().il_last_error()
  for (_, wrows, _, _, _), (gbuf, grows, _, _, _) in zip(want, got):
    assert torch.equal(_bits(grows), _bits(wrows))
    assert bool((gbuf[:GUARD + 1] == SENTINEL).all()) and bool((gbuf[GUARD + 1 + n * row:] == SENTINEL).all())


def test_mix_relabel_population_refusals():
  """Every refusal is IL_ERR_ARG with a text naming the entry point, and nothing is launched: the valid device array of a two-learner population stays behind every call,
  so a launch that went out anyway would edit its rows."""
  L_ = _lib.lib()
  dims, mode, n = (11, 3), (2, 3), 16
  learners, row, o_rew = _case(dims, mode, n, [n, n // 2], 3)
  dev = _device_side(learners)
  before = [buf.clone() for buf, *_ in dev]
  dyn = torch.stack([d[3] for d in dev]).contiguous()
  descs = il_training._device_array([_lib.MixLearner(rows.data_ptr(), erows.data_ptr(), dyn[l].data_ptr(), re) for l, (_, rows, erows, _, re) in enumerate(dev)], DEV)
  dd, S, A = _lib.ptr(descs), dims[0], dims[1]
  for args, word in (((None, 2, n, S, A, 2, 3), b'null'), ((dd, 0, n, S, A, 2, 3), b'n_learners=0'), ((dd, 65536, n, S, A, 2, 3), b'n_learners=65536'), ((dd, -1, n, S, A, 2, 3), b'n_learners=-1'),
                     ((dd, 2, 0, S, A, 2, 3), b'n=0'), ((dd, 2, -16, S, A, 2, 3), b'n=-16'), ((dd, 2, n, S, A, 3, 3), b'label=3'), ((dd, 2, n, S, A, -1, 3), b'label=-1'),
                     ((dd, 2, n, S, A, 2, 0), b'label=2 update_freq=0'), ((dd, 2, n, S, A, 2, -5), b'label=2 update_freq=-5')):
    assert L_.il_batch_mix_relabel_population(*args, _lib.stream_ptr()) == 1, word   # IL_ERR_ARG
    assert b'il_batch_mix_relabel_population' in L_.il_last_error() and word in L_.il_last_error(), (word, L_.il_last_error())
  torch.cuda.synchronize()
  assert all(torch.equal(_bits(buf), _bits(b)) for (buf, *_), b in zip(dev, before)), 'a refused call launched its kernel'
  _lib.check(L_.il_batch_mix_relabel_population(dd, 2, n, S, A, 2, 3, _lib.stream_ptr()))   # ... and the same array is served once the call is valid
  torch.cuda.synchronize()
  want = _per_learner(learners, n, dims, mode)
  assert all(torch.equal(_bits(g[0]), _bits(w[0])) for g, w in zip(dev, want))
  assert not torch.equal(_bits(dev[0][0]), _bits(before[0]))


# ---------------------------------------------------------------------------------------------
# il.BatchedPopulationPlan('AdRIL') against plan.relabel_args(...); plan.run() per learner
# ---------------------------------------------------------------------------------------------
def _adril_learners(n, update_freq, balanced, B=64, hidden=64, bc_aux=False):
  """n independent AdRIL / SQIL learners at hopper dims (own networks, rings, index streams, Philox counters, relabellers and expert trajectory counts) as UpdatePlans,
  reproducibly - built like the RED and DRIL population tests build theirs (gpu_util.fill_memory stamps the rows 1..1500). update_freq / balanced: one value or one per learner."""
  il_training._NOISE.clear(); il_training._WS.clear()
  plans, state = [], []
  S, A = gi.DIMS['hopper']
  per = lambda v: v if isinstance(v, (list, tuple)) else [v] * n
  for l in range(n):
    torch.manual_seed(60 + l)
    cfg = Cfg(hidden_size=hidden, depth=2, activation='relu')
    actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
    target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
    ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
    rs = np.random.RandomState(60 + l)
    mem = il.ReplayMemory(4000, S, A, True, device=DEV); fill_memory(mem, gi.transitions(rs, 1500, S, A), 1500)
    emem = il.ReplayMemory(600, S, A, True, device=DEV); fill_memory(emem, gi.transitions(rs, 600, S, A, state_shift=0.5), 600)
    emem.num_trajectories = 5 + 2 * l   # own 1 / |expert trajectories|
    mem.index_rng = emem.index_rng = il.IndexStream(100 + l)
    relabeller = il.RewardRelabeller(per(update_freq)[l], per(balanced)[l])
    plans.append(il.UpdatePlan('AdRIL', actor, critic, log_alpha, target, mem, ao, co, to, B, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=relabeller, overlap=False,
                               learner_id=l, bc_aux=bc_aux))
    state.append((actor, critic, target, log_alpha, ao, co, to, mem, relabeller))
  return plans, state


STEPS = (1001, 1002, 1003, 1004, 1005)   # update_freq 2: rounds 501, 501, 502, 502, 503 - the round changes inside the test; a third of the stamps 1..1500 are not older


def _relabel_inputs(u, n):
  return STEPS[u], [3 + l + 2 * u for l in range(n)]   # the step of update u and every learner's own, growing, trajectory count


def _adril_state(plans, state):
  torch.cuda.synchronize()
  out = []
  for l, ((actor, critic, target, log_alpha, ao, co, to, mem, relabeller), p) in enumerate(zip(state, plans)):
    counter = il_training._noise_counter(actor.flat.device, l)   # the learner's update counter (learner_id = l)
    out.append([N(actor.flat), N(critic.flat), N(target.flat), N(log_alpha)] + [N(t) for o in (ao, co, to) for t in (o.exp_avg, o.exp_avg_sq, o.step_count[:1])]
               + [N(_bits(p.rows)), N(_bits(p.transitions['rewards'])), N(p.logp), N(p.q), N(p.idx), N(p.eidx), N(mem.stream().device_state(DEV)), N(counter),
                  np.array([relabeller.sample_expert])])
  return out


def _rows_snapshot(plans):
  torch.cuda.synchronize()
  return [(N(_bits(p.rows)), N(_bits(p.erows))) for p in plans]


@pytest.mark.parametrize('how', ['eager', 'captured'])
@pytest.mark.parametrize('update_freq', [2, 0], ids=['AdRIL-freq2', 'SQIL'])
@pytest.mark.parametrize('balanced', [True, False], ids=['balanced', 'halves'])
def test_adril_population_plan_equals_plan_run_per_learner(balanced, update_freq, how):
  """Five updates of three learners: BatchedPopulationPlan (eager; or one eager run, capture(), four replays) with pop.relabel_args in front of every update against
  plan.relabel_args(...); plan.run() per learner - the rows and rewards after EVERY update through int32 views, then actor, critic, target, log_alpha, the optimisers'
  moments and step counts, logp, q, the drawn indices, the index-stream state, the noise counter and the relabeller's sample_expert flag, bit for bit."""
  n, updates = 3, len(STEPS)
  plans, state = _adril_learners(n, update_freq, balanced)
  want_rows = []
  for u in range(updates):
    step, counts = _relabel_inputs(u, n)
    for p, c in zip(plans, counts):
      p.relabel_args(step, c); p.run()
    want_rows.append(_rows_snapshot(plans))
  want = _adril_state(plans, state)
  plans, state = _adril_learners(n, update_freq, balanced)
  pop = il.BatchedPopulationPlan(plans)
  assert pop.algorithm == 'AdRIL' and pop.side is None and tuple(pop.dyn.shape) == (n, 3) and pop.dyn.dtype == torch.int64
  o_rew = 2 * plans[0].memory.state_size + plans[0].memory.action_size
  for u in range(updates):
    pop.relabel_args(*_relabel_inputs(u, n))
    if how == 'captured' and u > 0: pop.replay()
    else: pop.run()
    if how == 'captured' and u == 0:
      torch.cuda.synchronize()
      pop.capture()
    got_rows = _rows_snapshot(plans)
    for l in range(n):
      np.testing.assert_array_equal(got_rows[l][0], want_rows[u][l][0], err_msg=f'update {u}, learner {l}: rows')
      np.testing.assert_array_equal(got_rows[l][1], want_rows[u][l][1], err_msg=f'update {u}, learner {l}: expert rows')
      same = np.array_equal(np.delete(got_rows[l][0], o_rew, axis=1), np.delete(got_rows[l][1], o_rew, axis=1))   # every column but the relabelled one
      if balanced: assert same == (u % 2 == 0), f'update {u}, learner {l}: the expert turn (first) and the policy turn alternate'
      else: assert not same and np.array_equal(np.delete(got_rows[l][0], o_rew, axis=1)[:32], np.delete(got_rows[l][1], o_rew, axis=1)[:32])
      r = got_rows[l][0][:, o_rew].view(np.float32)
      if update_freq == 0:
        assert set(np.unique(r).tolist()) <= {0.0, 1.0}
      elif not balanced or u % 2 == 1:   # policy rows: the current round's -0.0 and the older rounds' -1 / trajectories both occur
        pol = r[32:] if not balanced else r
        assert (pol.view(np.int32) == -2 ** 31).any() and (pol == np.float32(-1) / np.float32(3 + l + 2 * u)).any() and (pol <= 0).all()
  got = _adril_state(plans, state)
  for l, (a_l, b_l) in enumerate(zip(want, got)):
    for i, (x, y) in enumerate(zip(a_l, b_l)):
      assert np.isfinite(x.astype(np.float64)).all()
      np.testing.assert_array_equal(x, y, err_msg=f'learner {l}, tensor {i}')
    assert int(a_l[20][0]) == updates, 'one bump of the noise counter per update'
    assert bool(a_l[21][0]) == (not balanced or updates % 2 == 0), 'a balanced relabeller flipped once per update; another one never'
  assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[0][13], want[1][13]), 'the learners are meant to differ'


def test_adril_population_plan_refusals():
  """Relabellers of different update_freq or balanced, bc_aux, and an eager run() that no relabel_args() preceded are refused; sub-populations take their own slices."""
  with pytest.raises(AssertionError, match='share batch, update_freq, balanced'):
    il.BatchedPopulationPlan(_adril_learners(2, [2, 3], True)[0])
  with pytest.raises(AssertionError, match='share batch, update_freq, balanced'):
    il.BatchedPopulationPlan(_adril_learners(2, 2, [True, False])[0])
  with pytest.raises(AssertionError, match='BC auxiliary step'):
    il.BatchedPopulationPlan(_adril_learners(2, 2, True, bc_aux=True)[0])
  pop = il.BatchedPopulationPlan(_adril_learners(2, 2, True)[0])
  with pytest.raises(AssertionError, match='relabel_args'):
    pop.run()
  pop.relabel_args(1001, [3, 4])
  pop.run()
  with pytest.raises(AssertionError, match='relabel_args'):   # ... and once per update
    pop.run()
  with pytest.raises(AssertionError, match='one trajectory count per learner'):
    pop.relabel_args(1002, [3])
  torch.cuda.synchronize()
  sub = il.BatchedPopulationPlan(_adril_learners(4, 2, True)[0], groups=2)
  sub.relabel_args(1001, [3, 4, 5, 6])
  assert [N(s.dyn)[:, 2].tolist() for s in sub.subs] == [[3, 4], [5, 6]] and all(s.side is None for s in sub.subs)


# ---------------------------------------------------------------------------------------------
# train.py -m seed=... algorithm=AdRIL +sweep.adril_population=true: population schedule against per_learner
# ---------------------------------------------------------------------------------------------
from test_train_gpu import COMMON  # noqa: E402  (steps 260, batch 64, two evaluations of two episodes, 60-step episodes)

ADRIL_10 = ['optimised_hyperparameters=AdRIL_10_trajectories', '+synthetic_env.dataset_trajectories=12']   # unbalanced, batch 128, 10 of the stand-in's 12 trajectories
SWEEP_CASES = [pytest.param([], id='shipped-balanced'), pytest.param(ADRIL_10, id='AdRIL_10-halves-batch128')]


def adril_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, short, tp, min_updates=2):
  """test_population_acting_gpu.sweep_schedules_leave_the_same_bytes for AdRIL (`tp`: that module): `-m seed=3,4` with the opt-in key under +sweep.schedule=population and
  per_learner - the same bytes in agent.pth and metrics.pth (timing keys aside), no discriminator.pth, different jobs, one population."""
  if any(a.startswith('optimised_hyperparameters=') for a in extra):   # the overlay's own batch size and dataset stand: later settings of the same keys would replace them
    short = [a for a in short if not a.startswith(('training.batch_size=', '+synthetic_env.dataset_trajectories='))]
  argv = ['-m', 'seed=3,4', 'algorithm=AdRIL', 'env=hopper', KEY] + short + extra
  roots = {}
  for schedule in ('population', 'per_learner'):
    capsys.readouterr()
    roots[schedule], scores = tp._sweep(tmp_path, schedule, argv + [f'+sweep.schedule={schedule}'])
    err = capsys.readouterr().err
    assert err.count('[train] sweep:') == 1 and 'train as one population of 2 learners' in err and f'+sweep.schedule={schedule}' in err, err
    assert np.isfinite(scores).all()
    roots[schedule + ' scores'] = scores
  assert roots['population scores'] == roots['per_learner scores']
  assert os.path.basename(os.path.dirname(roots['population'])) == 'AdRIL_hopper_sweeper'
  jobs = []
  for j in (0, 1):
    fp, fl = tp._job_files(roots['population'], j), tp._job_files(roots['per_learner'], j)
    assert set(fp) == set(fl) == {'agent.pth', 'metrics.pth'}, 'no discriminator.pth for AdRIL, as in train()'
    for f in fp:
      a, b = fp[f], fl[f]
      if f == 'metrics.pth':
        a, b = ({k: v for k, v in m.items() if k not in tp.TIMING_KEYS} for m in (a, b))
        assert len(a['update_steps']) >= min_updates and len(a['test_steps']) == 2 and all(np.isfinite(q).all() for q in a['Q_values'])
        assert all(float(np.max(r)) <= 1.0 and float(np.min(r)) >= -1.0 for r in a['predicted_rewards']), 'AdRIL rewards are +1 / |expert|, -0 or -1 / |policy|'
        if extra: assert all(q.shape == (128,) for q in a['Q_values'])
      tp._assert_same_nested(a, b, f'job {j}: {f}')
    assert all(torch.isfinite(v).all() for v in fp['agent.pth']['actor'].values())
    jobs.append(fp)
  assert any(not torch.equal(v, jobs[1]['agent.pth']['actor'][k]) for k, v in jobs[0]['agent.pth']['actor'].items()), 'the jobs of a seed sweep are meant to differ'
  assert jobs[0]['metrics.pth']['test_returns'] != jobs[1]['metrics.pth']['test_returns']


@pytest.mark.parametrize('extra', SWEEP_CASES)
def test_adril_seed_sweep_population_equals_per_learner(tmp_path, capsys, extra):
  import test_population_acting_gpu as tp
  adril_sweep_schedules_leave_the_same_bytes(tmp_path, capsys, extra, COMMON, tp)
