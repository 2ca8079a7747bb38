"""`-m gpu`: the Q pass and the counter bookkeeping taken off the last leg of the policy / critic launch. In k_policy_critic_quad the mask of the hidden layer's
backward, dz2 = w3 [h2 > 0], is written where h2 arrives - by the MFMA waves' forward epilogue for their own columns, by the hop's receive for the other quarters'
(mlp_tile.hpp quad_receive_each) - into a tile of its own, so that the backward GEMM starts behind the receive's barrier; Q = h2 . w3 + b3 is summed beside it by waves
4 .. 7 of quarter 0 alone, over the raw tile. In the helpers (policy_critic_helper, quad and pair launch) the returning count of the tile counter and its reset moved from
thread 0, whose wave issues the leg's first loads, to a thread of the last wave.

None of this changes an operation, an operand or a summation order, so the yardstick is bits, through the bodies of tests/test_tail_loads_gpu.py: six updates of a GAIL
plan through run(), launch_direct() and back-to-back launch_direct(join=False) - every counter is reused six times - against the stream-dependency schedule
(IL_DEVICE_SYNC=0) in this process and the 16-wave kernels (IL_PAIR=0, k_policy_critic's in-place pass) in a fresh process, update by update (log pi and min Q among the
compared arrays) and at the end.

Shapes, all at H = 256: B = 16 (one tile, the smallest quad), 48 (three tiles, plain decode), 128 (XCD-aware decode); widths (18, 6), (16, 8), (12, 3), (17, 6), (32, 8);
IL_QUAD=0 at B = 48: the helpers of the pair launch with the moved bookkeeping.
Value edges at B = 16, the critics' parameters set before the plan and the target copy are made:
  'dead'  critic 1's b2 is -100 on columns of every quarter (whole 16-column tiles, and every third column elsewhere): h2 is exactly 0 there behind a negative
          pre-activation, and the mask must be 0 - in the MFMA waves' own columns and in received ones.
  'tie'   critic 2 is a copy of critic 1: q1 == q2 on every row, the 0.5 branch of the min's derivative runs, and the two stay copies of each other.
One width is replayed through the numpy oracle at the bounds of tests/test_chain_legs_gpu.py.
The bodies take the parity module as an argument: tests/test_qpass_emulated.py runs them on the host emulation of the kernels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_chain_legs_gpu as G
import test_tail_loads_gpu as T

pytestmark = pytest.mark.gpu

ROOT = T.ROOT
H = 256
CASES = [(16, (18, 6)), (48, (18, 6)), (128, (18, 6)), (48, (16, 8)), (48, (12, 3)), (48, (17, 6)), (48, (32, 8))]
PAIR_LAUNCH_CASES = [(48, (18, 6))]
EDGES = ('dead', 'tie')
EDGE_B, EDGE_DIMS = 16, (18, 6)
ORACLE_DIMS = (16, 8)


def dead_columns():
  """Columns 16 .. 31 (one whole MFMA tile of quarter 0), 208 .. 223 (of quarter 3) and every third column: own and received columns of every quarter."""
  return sorted(set(range(16, 32)) | set(range(208, 224)) | set(range(0, H, 3)))


def install_edge(monkeypatch, tgp, edge):
  """TwinCritic as make_plan constructs it, with the parameters of the edge: the target network and the plan's lane-ordered copies are made from it afterwards."""
  il = tgp.il
  make = il.TwinCritic

  def twin_critic(S, A, cfg, device=None):
    c = make(S, A, cfg, device=device)
    IN, stride = S + A, c.net_stride
    o_b2 = H * IN + H + H * H   # W1 | b1 | W2 | b2 | W3 | b3
    assert stride >= o_b2 + H + H + 1 and next(c.critic_1.parameters()).numel() == H * IN
    with torch.no_grad():
      if edge == 'dead':
        c.flat[o_b2 + torch.tensor(dead_columns(), device=c.flat.device)] = -100.0
      elif edge == 'tie':
        c.flat[stride:2 * stride] = c.flat[:stride]
      else: raise ValueError(edge)
    return c
  monkeypatch.setattr(il, 'TwinCritic', twin_critic)


# A fresh process (a C-side switch in `env`) with the edge installed: six updates per mode, the digests of every compared array as one JSON line.
CODE = """
import sys, json; sys.path[:0] = ['.', 'tests', 'tests/golden']
import pytest
import test_gpu_parity as tgp
import test_chain_legs_gpu as G
import test_tail_loads_gpu as T
import test_qpass_gpu as Q
mp = pytest.MonkeyPatch()
Q.install_edge(mp, tgp, {edge!r})
out = {{}}
for mode in {modes!r}:
  out[mode] = T.digests(*G.six_updates(tgp, mp, {B}, {dims!r}, 256, True, mode))
mp.undo()
print(json.dumps(out))
"""


def fresh_process_with_edge(edge):
  def run(B, dims, modes, **env):
    r = subprocess.run([sys.executable, '-c', CODE.format(B=B, dims=tuple(dims), modes=tuple(modes), edge=edge)], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])
  return run


def check_edge_premise(tgp, monkeypatch, edge, B, dims):
  """What the edge is there for, read from the control's outputs: 'tie' - the critics are still copies of each other after six updates (q1 == q2 on every row of every
  update, or their gradients would have parted them); 'dead' - critic 1's b2 still holds -100 on the dead columns (no row ever had a positive pre-activation there)."""
  _, final = G.six_updates(tgp, monkeypatch, B, dims, H, True, 'control')
  critics, stride = final[1], final[1].size // 2
  if edge == 'tie':
    np.testing.assert_array_equal(critics[:stride], critics[stride:])
  else:
    o_b2 = H * sum(dims) + H + H * H
    np.testing.assert_array_equal(critics[o_b2 + np.array(dead_columns())], np.float32(-100.0))
    assert not (critics[stride + o_b2:stride + o_b2 + H] == np.float32(-100.0)).any()


def edge_equals_both_controls(tgp, monkeypatch, edge, run=None, B=EDGE_B, dims=EDGE_DIMS):
  """run(B, dims, modes, **env) -> {mode: digests} in a fresh process with the edge installed (default: this file's, on the GPU)."""
  run = run or fresh_process_with_edge(edge)
  install_edge(monkeypatch, tgp, edge)
  check_edge_premise(tgp, monkeypatch, edge, B, dims)
  T.bits_equal_both_controls(tgp, monkeypatch, B, dims, other_control=lambda B, dims: run(B, dims, ('run',), IL_PAIR='0')['run'])


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B,dims', CASES)
def test_six_updates_leave_the_bits_of_both_controls(monkeypatch, B, dims):
  import test_gpu_parity as tgp
  T.bits_equal_both_controls(tgp, monkeypatch, B, dims)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B,dims', PAIR_LAUNCH_CASES)
def test_helpers_of_the_pair_launch_leave_the_bits_of_both_controls(monkeypatch, B, dims):
  import test_gpu_parity as tgp
  T.pair_launch_equals_both_controls(tgp, monkeypatch, B, dims, T.fresh_process)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('edge', EDGES)
def test_value_edges_leave_the_bits_of_both_controls(monkeypatch, edge):
  import test_gpu_parity as tgp
  edge_equals_both_controls(tgp, monkeypatch, edge)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
def test_six_updates_replay_through_the_oracle(monkeypatch):
  import bench
  import test_timed_path_oracle as O
  T.width_replays_through_the_oracle(O, bench, monkeypatch, ORACLE_DIMS)
