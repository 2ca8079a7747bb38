"""`-m gpu`: actor(s') of the forward / critic-loss launch requests its rows ahead of its wait for the index draw (sac.hip actor_next_pair `spec`,
il_sac_update_gather_spec) from the private slab the sampler workgroup stages beside the dense one (mt_device.hpp MtStage.next, il_gail_disc_step_draw_staged2), and uses
them when the previous update's tail has seen the draw complete ([IL_SYNC_DRAW_SEEN], written by sac.hip dw_tail_alpha); otherwise it waits as before and asks again.

Nothing here changes an operation or its order, so the yardstick is bits, against the schedule that shares none of these waits (IL_DEVICE_SYNC=0: stream dependencies,
rows gathered by a kernel): eight updates through run(), launch_direct() and back-to-back launch_direct(join=False), per update and at the end. The vouched path is
driven deterministically (the side branch alone, then a true [IL_SYNC_DRAW_SEEN] stored by the host, then the main branch), the unvouched one with rows that really are
stale (IL_EARLY_DRAW=0: the chain launch is resident before the draw), and the real schedule must reach the vouched path on its own. The slab's contents are compared
with a host gather through the index array.
The bodies take the parity module as an argument: tests/test_spec_rows_emulated.py runs them on the host emulation of the kernels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inputs as gi
import test_chain_legs_gpu as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, (S, A), H): one tile; three tiles (plain role decode); the XCD-aware decode; state widths whose W1 rows are 16-byte aligned (16), 8-byte aligned with one
# straddling k-block (14), with a second k-block partly valid (18, 22) and odd (17) - the slab's row is S + 1 floats rounded up to 32 at every one of them;
# H = 64: k_sac_chain, which ignores the slab but runs behind the tail that writes [IL_SYNC_DRAW_SEEN]; the headline shape
SHAPES = [(16, (18, 6), 256), (48, (18, 6), 256), (128, (18, 6), 256), (48, (16, 6), 256), (48, (14, 6), 256), (48, (22, 6), 256), (48, (17, 6), 256), (48, (18, 6), 64),
          (256, (18, 6), 256)]
NAMES = ('discriminator parameters', 'u / v', 'relabelled rewards', 'log pi', 'min Q', 'index draw')


def make_plan(tgp, B, dims, H, absorbing=True, seed=21):
  """tests/test_chain_legs_gpu.py make_plan (spectral norm on) with the rings' absorbing-state flag as an argument."""
  if absorbing: return G.make_plan(tgp, B, dims, H, True, seed)
  il, DEV, Cfg = tgp.il, tgp.DEV, tgp.Cfg
  S, A = dims
  torch.manual_seed(seed)
  cfg = Cfg(hidden_size=H, depth=2, activation='relu')
  actor, critic = il.SoftActor(S, A, cfg, device=DEV), il.TwinCritic(S, A, cfg, device=DEV)
  target, log_alpha = il.create_target_network(critic), torch.zeros(1, device=DEV)
  ao, co, to = il.AdamW(actor, lr=3e-4, weight_decay=0), il.AdamW(critic, lr=3e-4, weight_decay=0), il.Adam(log_alpha, lr=3e-4)
  rs = np.random.RandomState(seed)
  tr, etr = gi.transitions(rs, 3000, S, A), gi.transitions(rs, 1000, S, A, state_shift=0.5)
  mem = il.ReplayMemory(8000, S, A, False, device=DEV); tgp.fill_memory(mem, tr, 3000)
  emem = il.ReplayMemory(1000, S, A, False, device=DEV); tgp.fill_memory(emem, etr, 1000)
  icfg = Cfg(state_only=False, spectral_norm=True, loss_function='BCE', grad_penalty=1.0, entropy_bonus=0.0, mixup_alpha=1, pos_class_prior=0.7, nonnegative_margin=float('inf'),
             discriminator=Cfg(hidden_size=64, depth=1, activation='relu', reward_shaping=False, subtract_log_policy=False, reward_function='AIRL'))
  disc = il.GAILDiscriminator(S, A, icfg, 0.97, device=DEV)
  do = il.AdamW(disc, lr=3e-5, weight_decay=10)
  plan = il.UpdatePlan('GAIL', actor, critic, log_alpha, target, mem, ao, co, to, B, 0.97, -0.5 * A, 0.99, expert_memory=emem, discriminator=disc, discriminator_optimiser=do,
                       imitation_cfg=icfg, device_index_draw=True)
  return plan, (actor, critic, target, log_alpha, disc)


def outputs(tgp, plan, disc):
  N = tgp.N
  return [N(disc.flat).copy(), N(disc.sn).copy(), N(plan.rewards).copy(), N(plan.logp).copy(), N(plan.q).copy(), N(plan.idx).copy()]


def finals(tgp, nets):
  return [tgp.N(n.flat if hasattr(n, 'flat') else n).copy() for n in nets]


def fresh_plan(tgp, monkeypatch, B, dims, H, control):
  monkeypatch.setenv('IL_DEVICE_SYNC', '0' if control else '1')
  monkeypatch.setenv('IL_STAGE_ROWS', '1'); monkeypatch.setenv('IL_SPEC_ROWS', '1')
  tgp.il.seed(41); tgp.il_training._NOISE.clear()
  plan, nets = make_plan(tgp, B, dims, H)
  if control: assert not plan.device_sync and not plan.ring_mode
  else: assert plan.device_sync and plan.ring_mode and plan.resident_sampler and plan.staged_rows and plan.spec_rows, 'the changed path: staged rows, the private slab, in-order launches'
  return plan, nets


def updates(tgp, monkeypatch, B, dims, H, mode, K=8):
  """mode 'control': stream dependencies; 'run': K run(); 'direct': two run(), then the recorded launches, joined; 'burst': the same back to back with no join in between
  (per-update outputs are not collected). Returns (per-update, final, launches that found their draw vouched for)."""
  plan, nets = fresh_plan(tgp, monkeypatch, B, dims, H, mode == 'control')
  per_update = []
  for k in range(K):
    if mode in ('direct', 'burst') and k == 2: plan.record_direct()
    if mode == 'burst' and k >= 2:
      plan.launch_direct(join=False)
      continue
    if mode == 'direct' and k >= 2:
      plan.launch_direct(); plan.join()
    else: plan.run()
    torch.cuda.synchronize()
    per_update.append(outputs(tgp, plan, nets[4]))
  plan.join(); torch.cuda.synchronize()
  assert plan.sync_timeouts() == 0 and not plan.poisoned()
  return per_update, finals(tgp, nets), (0 if mode == 'control' else plan.draw_vouched())


def compare(want, got, what):
  for k, (w, g) in enumerate(zip(want, got)):
    for name, a, b in zip(NAMES, w, g):
      assert np.isfinite(b).all()
      np.testing.assert_array_equal(a, b, err_msg=f'{what}: {name} of update {k}')


def bits_equal_the_control(tgp, monkeypatch, B, dims, H, modes=('run', 'direct', 'burst')):
  want_updates, want_final, _ = updates(tgp, monkeypatch, B, dims, H, 'control')
  for mode in modes:
    got_updates, got_final, vouched = updates(tgp, monkeypatch, B, dims, H, mode)
    print(f'B {B}, dims {dims}, H {H}, {mode}: {vouched} of 8 forward / critic-loss launches found their draw vouched for')
    compare(want_updates, got_updates, f'{mode}, B {B}, dims {dims}, H {H}')
    for i, (a, b) in enumerate(zip(want_final, got_final)):
      np.testing.assert_array_equal(a, b, err_msg=f'{mode}, B {B}, dims {dims}, H {H}: tensor {i} after eight updates')


def vouched_path_is_taken_and_leaves_the_bits(tgp, monkeypatch, B, K=6):
  """Update n, synchronise; the side branch of update n + 1 alone (its draw completes), synchronise; the host stores the [IL_SYNC_INDICES] it reads into
  [IL_SYNC_DRAW_SEEN] - a true statement by an agent that precedes the launch; the main branch: the launch counts itself vouched and leaves the control's bits."""
  want_updates, want_final, _ = updates(tgp, monkeypatch, B, (18, 6), 256, 'control', K)
  plan, nets = fresh_plan(tgp, monkeypatch, B, (18, 6), 256, False)
  got = []
  for k in range(K):
    if k == 2: plan.record_direct()
    if k < 2: plan.run()
    else:
      for fn, args in plan._direct_side: assert fn(*args) == 0
      plan.join(); torch.cuda.synchronize()
      drawn = int(plan.sync[plan._sync_indices].item())
      assert drawn == k + 1, 'the side branch alone has made this update\'s draw'
      plan.sync[plan._sync_draw_seen] = drawn
      before = plan.draw_vouched()
      torch.cuda.synchronize()
      for fn, args in plan._direct_main: assert fn(*args) == 0
      plan.join(); torch.cuda.synchronize()
      assert plan.draw_vouched() == before + 1, 'the launch behind a vouching word takes the rows it requested ahead of its wait'
    torch.cuda.synchronize()
    got.append(outputs(tgp, plan, nets[4]))
  assert plan.sync_timeouts() == 0 and not plan.poisoned()
  compare(want_updates, got, f'vouched, B {B}')
  for i, (a, b) in enumerate(zip(want_final, finals(tgp, nets))):
    np.testing.assert_array_equal(a, b, err_msg=f'vouched, B {B}: tensor {i} at the end')


def slab_holds_the_drawn_rows(tgp, monkeypatch, B, absorbing):
  """After a draw the private slab equals next_states and absorbing gathered through the index array, every pad column zero."""
  from imitation_learning_amd import memory as il_memory, _lib as il_lib
  monkeypatch.setenv('IL_DEVICE_SYNC', '1'); monkeypatch.setenv('IL_STAGE_ROWS', '1'); monkeypatch.setenv('IL_SPEC_ROWS', '1')
  tgp.il.seed(41); tgp.il_training._NOISE.clear()
  plan, _ = make_plan(tgp, B, (18, 6), 256, absorbing)
  assert plan.spec_rows
  N = tgp.N
  for _ in range(3):
    plan.run(); plan.join(); torch.cuda.synchronize()
    idx = N(plan.idx).astype(np.int64)
    views = il_memory.batch_views(plan.memory.ring, plan.memory.state_size, plan.memory.action_size, plan.memory.absorbing)
    S = plan.memory.state_size
    slab = N(plan.stage_next)
    assert slab.shape == (B, int(il_lib.lib().il_stage_next_row_floats(S))) and slab.shape[1] % 32 == 0 and slab.shape[1] >= S + 1
    np.testing.assert_array_equal(slab[:, :S], N(views['next_states'])[idx])
    np.testing.assert_array_equal(slab[:, S], N(views['absorbing'])[idx])
    assert not slab[:, S + 1:].any(), 'pad columns'
    if absorbing: assert N(views['absorbing']).any(), 'a ring with absorbing states in it'
    else: assert not slab[:, S].any()


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B,dims,H', SHAPES)
def test_eight_updates_leave_the_bits_of_the_stream_dependency_schedule(monkeypatch, B, dims, H):
  import test_gpu_parity as tgp
  bits_equal_the_control(tgp, monkeypatch, B, dims, H)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B', [16, 48])
def test_vouched_launch_uses_the_rows_requested_ahead_of_the_wait(monkeypatch, B):
  import test_gpu_parity as tgp
  vouched_path_is_taken_and_leaves_the_bits(tgp, monkeypatch, B)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B', [16, 48])
@pytest.mark.parametrize('absorbing', [True, False])
def test_private_slab_holds_next_states_and_absorbing_of_the_drawn_rows(monkeypatch, B, absorbing):
  import test_gpu_parity as tgp
  slab_holds_the_drawn_rows(tgp, monkeypatch, B, absorbing)


DRAW_CODE = """
import sys, json, hashlib, numpy as np, torch; sys.path[:0] = ['.', 'tests', 'tests/golden']
import imitation_learning_amd as il
from imitation_learning_amd import training as T
from test_gpu_parity import _make_plan, N
il.seed(31); T._NOISE.clear()
plan, nets = _make_plan('GAIL', 17, B={B})
for _ in range(2): plan.run()
plan.record_direct()
for _ in range(6): plan.launch_direct(join=False)     # back to back: the chain launch of update k + 1 is dispatched behind update k's tail
plan.join(); torch.cuda.synchronize()
h = hashlib.sha256()
for n in list(nets) + [plan.logp, plan.q, plan.rewards, plan.idx]: h.update(np.ascontiguousarray(N(n.flat if hasattr(n, 'flat') else n)).tobytes())
print(json.dumps(dict(digest=h.hexdigest(), timeouts=plan.sync_timeouts(), poisoned=plan.poisoned(), spec=plan.spec_rows, vouched=plan.draw_vouched())))
"""


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B', [256, 48])
def test_unvouched_launch_waits_and_asks_again_for_rows_that_were_stale(B):
  """IL_EARLY_DRAW=0: the sampler waits for the previous update's end, so that update's tail reads [IL_SYNC_INDICES] before the draw it could vouch for exists - no launch
  is ever vouched for - and the chain launch is resident before the draw: the rows it requested ahead of its wait are the previous draw's, and must be dropped.
  Equal digests with IL_EARLY_DRAW=1, no expired wait."""
  outs = []
  for value in ('1', '0'):
    r = subprocess.run([sys.executable, '-c', DRAW_CODE.format(B=B)], env=dict(os.environ, IL_EARLY_DRAW=value, IL_STAGE_ROWS='1', IL_SPEC_ROWS='1'), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
  print(outs)
  for o in outs:
    assert o['timeouts'] == 0 and not o['poisoned'] and o['spec'], o
  assert outs[1]['vouched'] == 0, 'IL_EARLY_DRAW=0: the tail cannot have seen the draw'
  assert outs[0]['digest'] == outs[1]['digest'], outs


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
def test_back_to_back_launches_reach_the_vouched_path(monkeypatch):
  """32 back-to-back direct launches at the headline batch size: the control's bits, and at least one launch found its draw vouched for by the previous update's tail
  (that the path is reached - its share of a timed run is a measurement, profiles/spec_rows.txt)."""
  import test_gpu_parity as tgp
  _, want_final, _ = updates(tgp, monkeypatch, 256, (18, 6), 256, 'control', 34)
  _, got_final, vouched = updates(tgp, monkeypatch, 256, (18, 6), 256, 'burst', 34)
  print(f'{vouched} of 34 forward / critic-loss launches found their draw vouched for')
  for i, (a, b) in enumerate(zip(want_final, got_final)):
    np.testing.assert_array_equal(a, b, err_msg=f'tensor {i} after 34 updates')
  assert vouched >= 1


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
def test_replays_of_a_plan_captured_at_its_first_update_leave_the_bits(monkeypatch):
  """A plan whose FIRST update is the captured one (capture(warmup=0)): whatever the host layer issues while it builds its descriptors is captured with it and runs
  again at the head of every replay. The private slab is therefore allocated without a fill - a captured fill cleared it under the chain launch that was still reading
  it. 300 back-to-back replays at the headline batch size against the stream-dependency schedule, captured the same way."""
  import test_gpu_parity as tgp
  results = []
  for control in (True, False):
    plan, nets = fresh_plan(tgp, monkeypatch, 256, (18, 6), 256, control)
    plan.capture(warmup=0)
    for _ in range(300): plan.replay()
    plan.join(); torch.cuda.synchronize()
    assert plan.sync_timeouts() == 0 and not plan.poisoned()
    results.append(finals(tgp, nets) + [tgp.N(plan.idx).copy(), tgp.N(plan.logp).copy(), tgp.N(plan.rewards).copy()])
    if not control:
      print(f'{plan.draw_vouched()} of 300 replays found their draw vouched for')
      assert plan.draw_vouched() >= 1
  for i, (a, b) in enumerate(zip(*results)):
    assert np.isfinite(b).all()
    np.testing.assert_array_equal(a, b, err_msg=f'tensor {i} after 300 replays')
