"""Quad mode of the policy / critic launch (k_policy_critic_quad) on the host emulation of the kernels (tests/host_emu): the emulator runs co-resident
workgroups as fibers, so the four-way hop between the quarters of a (tile, critic) - announces, write-through stores, flags, the third consumer clearing a line - runs here
as it does on the GPU. IL_QUAD is read once per process: the switch is compared through subprocesses."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402

NT = 256 // 16   # the headline batch's row tiles; the emulator reports 256 CUs: (8 + 4) * NT + 60 fit


def test_headline_updates_on_the_emulated_kernels(monkeypatch):
  """Three updates of the headline plan (two direct, one graph replay) with the default switches: no wait expired, the quad launch ran (its grid in the launch stamps).
  With IL_QUAD_EMU_DIGEST set, the digest of the learner and the policy / critic grid are written there (the switch comparison below)."""
  import torch
  tgp = E._emulated_product(monkeypatch, streams=True)
  tt, bench = E._timed_path_modules(monkeypatch, tgp)
  plan, nets, _ = bench.build(torch.device('cpu'), 0, seed=9)
  _lib.check(_lib.lib().il_kernel_stamps_clear())
  for _ in range(2): plan.run()
  plan.capture(warmup=0)
  plan.replay()
  plan.join()
  assert plan.sync_timeouts() == 0 and not plan.poisoned()
  wgs = _lib.kernel_stamps()['k_policy_critic_pair']['workgroups']
  h = hashlib.sha256()
  for n in list(nets) + [plan.logp, plan.q, plan.rewards, plan.idx]:
    a = (n.flat if hasattr(n, 'flat') else n).detach().cpu().numpy()
    assert np.isfinite(a).all()
    h.update(np.ascontiguousarray(a).tobytes())
  out = os.environ.get('IL_QUAD_EMU_DIGEST')
  if out:
    with open(out, 'w') as f: json.dump(dict(digest=h.hexdigest(), workgroups=wgs), f)
  if os.environ.get('IL_QUAD', '1') != '0':
    assert wgs == (8 + 4) * NT, wgs


def test_quad_switch_is_bit_identical_on_the_emulated_kernels(tmp_path):
  got = {}
  for v in ('1', '0'):
    out = str(tmp_path / f'quad{v}.json')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider', os.path.abspath(__file__) + '::test_headline_updates_on_the_emulated_kernels'],
                       env=dict(os.environ, IL_QUAD=v, IL_QUAD_EMU_DIGEST=out), cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    with open(out) as f: got[v] = json.load(f)
  assert got['1']['workgroups'] == (8 + 4) * NT and got['0']['workgroups'] == (4 + 4) * NT, got
  assert got['1']['digest'] == got['0']['digest'], got
