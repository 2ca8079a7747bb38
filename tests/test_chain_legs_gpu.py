"""`-m gpu`: the two legs of the forward / critic-loss launch and their join: the launch's wait for the index draw with both sync words in one batch and,
for actor(s'), behind the weight requests (sac.hip actor_next_pair, il_common.hpp sync_wait's split form); the discriminator's policy / expert calls without the wait for the previous update's end and its mixing call with the rows requested ahead of it (gail.hip).

None of this changes an operation or its order, so the yardstick is bits: six consecutive updates - every counter and flag line is reused several times -
through UpdatePlan.run() and through launch_direct(), against the schedule that shares none of the changed code paths' waits: IL_DEVICE_SYNC=0 (stream dependencies, rows
gathered by a kernel, the stand-alone reward kernel - the per-function launches in the reference loop's order), update by update for the discriminator's parameters, u / v
and the relabelled rewards, and for every persistent tensor at the end. The headline learner at B = 256, 48 and 16 is also replayed through the numpy oracle (tests/test_timed_path_oracle.py), with the
gradient penalty's coefficients drawn from Philox and given. Not run by these files: the device-sync gathered path (IL_RING_GATHER=0, [IL_SYNC_ROWS]), whose code is unchanged.
The bodies take the parity module as an argument: tests/test_chain_legs_emulated.py runs them on the host emulation of the kernels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inputs as gi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, (S, A), H): one tile; three tiles (the plain role decode) at state widths 18 and 16 - actor(s')'s first layer through LDS / from register lanes (l1_rows_aligned);
# 128 and 256 rows: the XCD-aware decode, pair mode and the quad launch beside it; H = 64: k_sac_chain, which shares the wait
SHAPES = [(16, (18, 6), 256), (48, (18, 6), 256), (48, (16, 6), 256), (128, (18, 6), 256), (256, (18, 6), 256), (48, (18, 6), 64)]


def make_plan(tgp, B, dims, H, spectral_norm, seed=21):
  """tests/test_gpu_parity.py _make_plan with the hidden width and the spectral norm as arguments."""
  il, DEV, Cfg = tgp.il, tgp.DEV, tgp.Cfg
  S, A = dims
  torch.manual_seed(seed)
  cfg = Cfg(hidden_size=H, depth=2, activation='relu')
  actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
  target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
  ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
  rs = np.random.RandomState(seed)
  tr, etr = gi.transitions(rs, 3000, S, A), gi.transitions(rs, 1000, S, A, state_shift=0.5)
  mem = il.ReplayMemory(8000, S, A, True, device=DEV); tgp.fill_memory(mem, tr, 3000)
  emem = il.ReplayMemory(1000, S, A, True, device=DEV); tgp.fill_memory(emem, etr, 1000)
  icfg = Cfg(state_only=False, spectral_norm=spectral_norm, loss_function='BCE', grad_penalty=1.0, entropy_bonus=0.0, mixup_alpha=1, pos_class_prior=0.7, nonnegative_margin=float('inf'),
             discriminator=Cfg(hidden_size=64, depth=1, activation='relu', reward_shaping=False, subtract_log_policy=False, reward_function='AIRL'))
  disc = il.GAILDiscriminator(S, A, icfg, 0.97, device=DEV)
  do = il.AdamW(disc, lr=3e-5, weight_decay=10)
  plan = il.UpdatePlan('GAIL', actor, critic, log_alpha, target, mem, ao, co, to, B, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=disc, discriminator_optimiser=do,
                       imitation_cfg=icfg, device_index_draw=True)
  return plan, (actor, critic, target, log_alpha, disc)


def six_updates(tgp, monkeypatch, B, dims, H, spectral_norm, mode, staged='1'):
  """mode 'control': stream dependencies; 'run': six run(); 'direct': two run(), then the recorded launches four times; 'burst': the same, back to back with no
  synchronisation or join in between - the discriminator launch of update k + 1 is then resident while update k still runs, which is when a Philox counter read
  ahead of the wait for the previous update's end would be the previous update's (per-update outputs are not collected). staged: IL_STAGE_ROWS - the chain launch reads its
  rows from the sampler's dense slab ('1', the default) or through the indices ('0'). Returns (per-update, final) arrays."""
  N = tgp.N
  monkeypatch.setenv('IL_DEVICE_SYNC', '0' if mode == 'control' else '1')
  monkeypatch.setenv('IL_STAGE_ROWS', staged)
  tgp.il.seed(41); tgp.il_training._NOISE.clear()
  plan, nets = make_plan(tgp, B, dims, H, spectral_norm)
  disc = nets[4]
  if mode == 'control': assert not plan.device_sync and not plan.ring_mode
  else:   # (H = 64: the critic-loss workgroups' spare LDS has no room for the discriminator, the stand-alone reward kernel runs)
    assert plan.device_sync and plan.ring_mode and plan.resident_sampler and plan.inline_relabel == (H == 256) and plan.staged_rows == (staged == '1'), 'the changed path: device hand-offs, rows through the rings, the in-launch sampler, inline relabel'
  per_update = []
  for k in range(6):
    if mode in ('direct', 'burst') and k == 2: plan.record_direct()
    if mode == 'burst' and k >= 2:
      plan.launch_direct(join=False)
      continue
    if mode == 'direct' and k >= 2:
      plan.launch_direct(); plan.join()
    else: plan.run()
    torch.cuda.synchronize()
    per_update.append([N(disc.flat).copy(), N(disc.sn).copy(), N(plan.rewards).copy(), N(plan.logp).copy(), N(plan.q).copy(), N(plan.idx).copy()])
  plan.join(); torch.cuda.synchronize()
  assert plan.sync_timeouts() == 0 and not plan.poisoned()
  return per_update, [N(n.flat if hasattr(n, 'flat') else n).copy() for n in nets]


def legs_equal_the_control(tgp, monkeypatch, B, dims, H, spectral_norm):
  want_updates, want_final = six_updates(tgp, monkeypatch, B, dims, H, spectral_norm, 'control')
  for mode, staged in (('run', '0'), ('direct', '1'), ('burst', '1')):   # rows through the indices (index -> row behind the wait) and from the staged slab
    got_updates, got_final = six_updates(tgp, monkeypatch, B, dims, H, spectral_norm, mode, staged)
    for k, (w, g) in enumerate(zip(want_updates, got_updates)):
      for name, a, b in zip(('discriminator parameters', 'u / v', 'relabelled rewards', 'log pi', 'min Q', 'index draw'), w, g):
        assert np.isfinite(b).all()
        np.testing.assert_array_equal(a, b, err_msg=f'{mode}, B {B}, dims {dims}, H {H}, spectral norm {spectral_norm}: {name} of update {k}')
    for i, (a, b) in enumerate(zip(want_final, got_final)):
      np.testing.assert_array_equal(a, b, err_msg=f'{mode}: tensor {i} after six updates')


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B,dims,H', SHAPES)
def test_six_updates_leave_the_bits_of_the_stream_dependency_schedule(monkeypatch, B, dims, H):
  import test_gpu_parity as tgp
  legs_equal_the_control(tgp, monkeypatch, B, dims, H, True)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B', [16, 48, 256])
def test_discriminator_calls_without_spectral_norm(monkeypatch, B):
  import test_gpu_parity as tgp
  legs_equal_the_control(tgp, monkeypatch, B, (18, 6), 256, False)


def headline_updates_against_the_oracle(O, bench, monkeypatch, given_eps, B=256):
  """The headline learner (bench.build; B other than 256: the same learner at that batch size - one tile, three tiles), six updates; after every update the index draws, the relabelled rewards (against the float64 bracket as well), log pi and min Q
  against the oracle's replay of the same updates, and the discriminator's parameters and u / v; its moments and every SAC tensor at the end. O: tests/test_timed_path_oracle.py
  (on the emulator: with its device names bound to the host).
  given_eps False: the timed schedule - two run(), four launch_direct(); the gradient penalty's coefficients drawn from Philox behind the wait for the previous update's end.
  given_eps True: the coefficients GIVEN (il_gail_disc_step's eps_gp; the launch with the in-launch sampler takes none, so the draw runs on the main stream,
  IL_RESIDENT_SAMPLER=0, and the discriminator step is issued here with the plan's descriptors): d.sync set, ring batches - the hand-off branch of k_gail_grad with
  mix_eps's `given` side, the Philox counter unread. Fresh uniforms every update, NOT the ones Philox would have drawn, fed to the oracle as well."""
  import ctypes as C
  from oracle import philox
  O.il_training._NOISE.clear(); O.il_training._WS.clear()
  if given_eps: monkeypatch.setenv('IL_RESIDENT_SAMPLER', '0')
  monkeypatch.setattr(bench, 'B', B); monkeypatch.setattr(O, 'B', B)   # (bench.build's and the oracle twin's batch size)
  plan, nets, (tr, et) = bench.build(torch.device(O.DEV), 0, seed=6)
  o = O.OracleLearner(nets, plan, tr, et, index_seed=6)
  assert plan.B == B and plan.device_sync and plan.ring_mode and plan.inline_relabel and plan.resident_sampler == (not given_eps)
  if given_eps:
    _lib = O._lib
    eps, rs, given = torch.zeros(O.B, device=O.DEV), np.random.RandomState(77), {}
    def disc_step(flags):
      rp, re_ = plan._ring_batches()
      _lib.check(_lib.lib().il_gail_disc_step(C.byref(plan.disc), C.byref(rp), C.byref(re_), _lib.ptr(eps), None, flags, _lib.stream_ptr()))
    monkeypatch.setattr(plan, '_disc_step', disc_step)
    recorded = O.record_noise
    monkeypatch.setattr(O, 'record_noise', lambda seed, ctr, stream_id, n: given[ctr] if stream_id == philox.STREAM_GP else recorded(seed, ctr, stream_id, n))
  for k in range(6):
    if given_eps:
      given[k] = rs.random_sample(O.B).astype(np.float32)
      assert not np.array_equal(given[k], recorded(o.key, k, philox.STREAM_GP, O.B))
      eps.copy_(torch.from_numpy(given[k])); torch.cuda.synchronize()
    if not given_eps and k == 2: plan.record_direct()
    if not given_eps and k >= 2:
      plan.launch_direct(); plan.join()
    else: plan.run()
    torch.cuda.synchronize()
    got = O.per_update_outputs(plan)
    O.compare_outputs(got, o.update(k), k)
    O.reward_bracket(o, nets[4], got[2], k)
    O.close(O.N(nets[4].flat), o.ds.pack(), f'discriminator after update {k}', atol_scale=4e-6 * (k + 1))
    for nm, val in nets[4].views().items():
      O.close(O.N(val), getattr(o.ds, nm), f'{nm} after update {k}', atol_scale=4e-6 * (k + 1))
  assert plan.sync_timeouts() == 0 and not plan.poisoned()
  O.compare_learner(o, nets, plan, 6)


ORACLE_CASES = [(256, False), (256, True), (48, False), (48, True), (16, False)]   # (B, eps_gp given)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B,given_eps', ORACLE_CASES)
def test_six_headline_updates_replay_through_the_oracle(monkeypatch, B, given_eps):
  import bench
  import test_timed_path_oracle as O
  headline_updates_against_the_oracle(O, bench, monkeypatch, given_eps, B)


DRAW_CODE = """
import sys, json, hashlib, numpy as np, torch; sys.path[:0] = ['.', 'tests', 'tests/golden']
import imitation_learning_amd as il
from imitation_learning_amd import training as T
from test_gpu_parity import _make_plan, N
il.seed(31); T._NOISE.clear()
plan, nets = _make_plan('GAIL', 17, B={B})
for _ in range(2): plan.run()
plan.record_direct()
for _ in range(4): plan.launch_direct(join=False)     # back to back: the chain launch of update k + 1 is dispatched behind update k's tail
plan.join(); torch.cuda.synchronize()
h = hashlib.sha256()
for n in list(nets) + [plan.logp, plan.q, plan.rewards, plan.idx]: h.update(np.ascontiguousarray(N(n.flat if hasattr(n, 'flat') else n)).tobytes())
print(json.dumps(dict(digest=h.hexdigest(), timeouts=plan.sync_timeouts(), poisoned=plan.poisoned(), ring=plan.ring_mode, inline=plan.inline_relabel)))
"""


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B,staged', [(256, '1'), (256, '0'), (48, '0')])
def test_both_arrival_orders_of_the_draw(B, staged):
  """IL_EARLY_DRAW=1: the indices exist long before the chain launch starts and its first look at the requested word ends the wait; IL_EARLY_DRAW=0: the sampler waits
  for the previous update's end, the chain launch is resident before the indices exist and the poll loop really spins. Equal digests, no expired wait. staged '0':
  the rows go through the indices, so a row index requested ahead of the wait would read the previous draw."""
  outs = []
  for value in ('1', '0'):
    r = subprocess.run([sys.executable, '-c', DRAW_CODE.format(B=B)], env=dict(os.environ, IL_EARLY_DRAW=value, IL_STAGE_ROWS=staged), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
  for o in outs:
    assert o['timeouts'] == 0 and not o['poisoned'] and o['ring'] and o['inline'], o
  assert outs[0]['digest'] == outs[1]['digest'], outs
