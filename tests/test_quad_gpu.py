"""`-m gpu`: quad mode of the policy / critic launch (k_policy_critic_quad: four workgroups per (tile, critic) instead of the pair launch's two) moves output
tiles between workgroups and nothing else: IL_QUAD=0 (the pair launch) and the default must not differ in a bit, at batch 256 (quad) and at batch 512, where the quad
launch exceeds its co-residency budget and the pair launch runs either way. The C-side switch is read once per process: compared through subprocesses."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = """
import sys, json, hashlib, numpy as np, torch; sys.path[:0] = ['.', 'tests', 'tests/golden']
import imitation_learning_amd as il
from imitation_learning_amd import training as T, _lib
from test_gpu_parity import _make_plan, N
il.seed(31); T._NOISE.clear()
plan, nets = _make_plan('GAIL', 17, B={B})
h = hashlib.sha256()
def fold():
  torch.cuda.synchronize()
  for n in list(nets) + [plan.logp, plan.q, plan.rewards, plan.idx]: h.update(np.ascontiguousarray(N(n.flat if hasattr(n, 'flat') else n)).tobytes())
for _ in range({K}): plan.run()       # direct launches, back to back
fold()
_lib.check(_lib.lib().il_kernel_stamps_clear())
plan.capture(warmup=0)
for _ in range({K}): plan.replay()    # graph replays, back to back
fold()
st = _lib.kernel_stamps()
print(json.dumps(dict(digest=h.hexdigest(), pc_workgroups=st['k_policy_critic_pair']['workgroups'], timeouts=plan.sync_timeouts(), poisoned=plan.poisoned())))
"""


def _run(B, quad, K=40):
  r = subprocess.run([sys.executable, '-c', CODE.format(B=B, K=K)], env=dict(os.environ, IL_QUAD=quad), cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('B', [256, 512])
def test_quad_switch_is_bit_identical(B):
  on, off = _run(B, '1'), _run(B, '0')
  nt = B // 16
  for o in (on, off):
    assert o['timeouts'] == 0 and not o['poisoned'], o
  assert off['pc_workgroups'] == (4 + 4) * nt, off   # the pair launch: 4 critic workgroups + 4 helpers per tile
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  quad_fits = (8 + 4) * nt + 60 <= cus   # sac.hip policy_critic_quad_ok: IL_QUAD_CU_RESERVE = 60
  assert on['pc_workgroups'] == ((8 + 4) * nt if quad_fits else (4 + 4) * nt), (on, cus)
  if B == 256 and cus >= 256:
    assert quad_fits, 'the headline batch runs the quad launch on an MI355X'
  assert on['digest'] == off['digest']


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
def test_quad_updates_beside_a_copy_hammering_process_equal_the_quiet_pair_run():
  """profiles/tools/soak_with_idle_parent.py (the learner as the child of a process with an idle GPU context, a neighbour process copying 256 MiB buffers back to back):
  20 000 updates of the headline schedule with the quad launch beside the copies against the quiet run, and the quiet runs of both launches against each other. The learner
  asserts that no device-side wait expired."""
  r = subprocess.run([sys.executable, os.path.join('profiles', 'tools', 'soak_with_idle_parent.py'), '20000', '1', 'IL_SOAK_LAUNCH=direct,IL_QUAD=1',
                      'IL_SOAK_LAUNCH=direct,IL_QUAD=0'], cwd=ROOT, capture_output=True, text=True, timeout=900)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = [l for l in r.stdout.splitlines() if 'mismatches' in l]
  assert len(lines) == 2, r.stdout[-2000:]
  quiet = [re.search(r'quiet (\S+);', l).group(1) for l in lines]
  assert not any(q.startswith('FAILED') for q in quiet), r.stdout[-2000:]
  assert quiet[0] == quiet[1], lines
  assert 'mismatches 0 / 1' in lines[0], lines
