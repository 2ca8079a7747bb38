"""`-m gpu`: the loads and MFMAs taken out from behind the last waits of the SAC update's two critical legs: the policy-backward helpers' W3 operands and
second h2 lanes requested ahead of their wait for the critics (mlp_tile.hpp tile_bwd_dx_prefetch, sac.hip actor_bwd_tile's PARK form), and the target critics' first
layer cut in two around the wait for a' (l1_compute_*_begin / _finish, target_pair). actor(s')'s head - whose bias lane was requested early too, measured and taken out
again, profiles/tail_loads.txt - runs between the two and is compared with them.

None of this changes an operation, an operand or a summation order, so the yardstick is bits: six updates of a GAIL plan through run(), launch_direct() and back-to-back
launch_direct(join=False) against two controls that share none of the changed code - the stream-dependency schedule (IL_DEVICE_SYNC=0, per-function launches) in this
process and the 16-wave kernels (IL_PAIR=0) in a subprocess, since that switch is read once per process - update by update for the discriminator's parameters, u / v,
the relabelled rewards, log pi, min Q and the index draw, and for actor, critics, targets, log alpha and discriminator at the end. One case per state / action width is
also replayed through the numpy oracle at the bounds of tests/test_chain_legs_gpu.py.

Widths (S, A), all at H = 256 (pair mode):
  (18, 6)  the headline: one k-block of the targets' first layer is s' alone, one straddles s' and a'
  (16, 8)  the second k-block is a' alone; 2A = 16: the FULL form of tile_bwd_dx
  (14, 6)  S < 16: nothing runs ahead of the wait
  (12, 3)  2A = 6
  (17, 6)  S + A odd: the critics' first layer through LDS
  (32, 8)  two whole s' k-blocks, Kpad = 48
Batch sizes: 16 (one tile), 48 (three tiles, plain decode), 128 (XCD-aware decode); IL_QUAD=0 at 48: the helpers of the pair launch.
The bodies take the parity module as an argument: tests/test_tail_loads_emulated.py runs them on the host emulation of the kernels."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_chain_legs_gpu as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256
WIDTHS = [(18, 6), (16, 8), (14, 6), (12, 3), (17, 6), (32, 8)]
# every width at three tiles; the headline width at one tile and at eight; the FULL form and Kpad = 48 once more at the other decode / tile count
CASES = [(48, w) for w in WIDTHS] + [(16, (18, 6)), (128, (18, 6)), (128, (16, 8)), (16, (32, 8))]
PAIR_LAUNCH_CASES = [(48, (18, 6)), (48, (16, 8)), (48, (12, 3))]   # IL_QUAD=0: clamped, FULL and narrow forms of the helpers' first GEMM
NAMES = ('discriminator parameters', 'u / v', 'relabelled rewards', 'log pi', 'min Q', 'index draw')
FINAL = ('actor', 'critics', 'targets', 'log alpha', 'discriminator')
MODES = ('run', 'direct', 'burst')


def digest(a):
  return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(per_update, final):
  return dict(updates=[[digest(a) for a in u] for u in per_update], final=[digest(a) for a in final])


def compare_arrays(want, got, what):
  (want_updates, want_final), (got_updates, got_final) = want, got
  for k, (w, g) in enumerate(zip(want_updates, got_updates)):
    for name, a, b in zip(NAMES, w, g):
      assert np.isfinite(b).all()
      np.testing.assert_array_equal(a, b, err_msg=f'{what}: {name} of update {k}')
  assert len(want_final) == len(got_final) == len(FINAL)
  for name, a, b in zip(FINAL, want_final, got_final):
    assert np.isfinite(b).all()
    np.testing.assert_array_equal(a, b, err_msg=f'{what}: {name} after six updates')


def compare_digests(want, got, what, per_update=True):
  if per_update:
    assert len(got['updates']) == 6
    for k, (w, g) in enumerate(zip(want['updates'], got['updates'])):
      for name, a, b in zip(NAMES, w, g):
        assert a == b, f'{what}: {name} of update {k}'
  for name, a, b in zip(FINAL, want['final'], got['final']):
    assert a == b, f'{what}: {name} after six updates'


# A fresh process (a C-side switch in `env`): six updates per mode, the digests of every compared array as one JSON line.
CODE = """
import sys, json; sys.path[:0] = ['.', 'tests', 'tests/golden']
import pytest
import test_gpu_parity as tgp
import test_chain_legs_gpu as G
import test_tail_loads_gpu as T
mp = pytest.MonkeyPatch()
out = {{}}
for mode in {modes!r}:
  out[mode] = T.digests(*G.six_updates(tgp, mp, {B}, {dims!r}, 256, True, mode))
mp.undo()
print(json.dumps(out))
"""


def fresh_process(B, dims, modes, **env):
  r = subprocess.run([sys.executable, '-c', CODE.format(B=B, dims=tuple(dims), modes=tuple(modes))], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  return json.loads(r.stdout.strip().splitlines()[-1])


_sixteen_wave = {}


def sixteen_wave_control(B, dims):
  """IL_PAIR=0: k_sac_chain and k_policy_critic, the 16-wave workgroups that pair mode splits - none of actor_next_pair, target_pair or the helpers. Once per shape."""
  key = (B, tuple(dims))
  if key not in _sixteen_wave: _sixteen_wave[key] = fresh_process(B, dims, ('run',), IL_PAIR='0')['run']
  return _sixteen_wave[key]


def bits_equal_both_controls(tgp, monkeypatch, B, dims, other_control=sixteen_wave_control):
  want = G.six_updates(tgp, monkeypatch, B, dims, H, True, 'control')
  want_d = digests(*want)
  compare_digests(want_d, other_control(B, dims), f'the two controls, B {B}, dims {dims}')
  for mode in MODES:
    got = G.six_updates(tgp, monkeypatch, B, dims, H, True, mode)
    compare_arrays((want[0] if mode != 'burst' else [], want[1]), got, f'{mode}, B {B}, dims {dims}')


def pair_launch_equals_both_controls(tgp, monkeypatch, B, dims, changed, other_control=sixteen_wave_control):
  """changed(B, dims, modes, IL_QUAD='0') -> {mode: digests}: the policy / critic launch as pairs, its helpers running the same PARK form behind four arrivals."""
  want_d = digests(*G.six_updates(tgp, monkeypatch, B, dims, H, True, 'control'))
  compare_digests(want_d, other_control(B, dims), f'the two controls, B {B}, dims {dims}')
  got = changed(B, dims, MODES, IL_QUAD='0')
  for mode in MODES:
    compare_digests(want_d, got[mode], f'IL_QUAD=0, {mode}, B {B}, dims {dims}', per_update=mode != 'burst')


def width_replays_through_the_oracle(O, bench, monkeypatch, dims, B=48):
  """tests/test_chain_legs_gpu.py's replay of six updates of the headline learner (two run(), four launch_direct(); its bounds), at another state / action width."""
  S, A = dims
  for m in (O, bench):
    monkeypatch.setattr(m, 'S', S); monkeypatch.setattr(m, 'A', A)
  monkeypatch.setattr(O, 'ENT', -0.5 * A)   # (the oracle twin's entropy target: bench.build's -0.5 A)
  G.headline_updates_against_the_oracle(O, bench, monkeypatch, False, B)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B,dims', CASES)
def test_six_updates_leave_the_bits_of_both_controls(monkeypatch, B, dims):
  import test_gpu_parity as tgp
  bits_equal_both_controls(tgp, monkeypatch, B, dims)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B,dims', PAIR_LAUNCH_CASES)
def test_helpers_of_the_pair_launch_leave_the_bits_of_both_controls(monkeypatch, B, dims):
  import test_gpu_parity as tgp
  pair_launch_equals_both_controls(tgp, monkeypatch, B, dims, fresh_process)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('dims', WIDTHS)
def test_six_updates_replay_through_the_oracle_at_every_width(monkeypatch, dims):
  import bench
  import test_timed_path_oracle as O
  width_replays_through_the_oracle(O, bench, monkeypatch, dims)
