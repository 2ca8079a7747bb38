"""The bodies of tests/test_chain_legs_gpu.py on the host emulation of the kernels (tests/host_emu): co-resident workgroups as fibers, so the chain launch's wait with its
first poll requested ahead and the discriminator calls' two waits run here as they do on the GPU. The emulator's reversed schedule (lane order, wave order between two
barriers, workgroup dispatch order, which stream runs next) is what catches a polling wave that depends on another wave's progress or a row index requested ahead of its
wait; IL_EMU_SCHEDULE, IL_EARLY_DRAW and IL_STAGE_ROWS are read once per process: compared through subprocesses. What the emulator cannot show: a Philox counter read
ahead of the wait for the previous update's end - its caller's stream is synchronous, the previous update has ended before the next discriminator launch is enqueued
(the GPU file's back-to-back mode catches that)."""
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
import test_chain_legs_gpu as G  # noqa: E402

# the GPU file's shapes - one tile; three tiles at both first-layer paths of actor(s'); k_sac_chain (H = 64); 8 and 16 tiles: the XCD-aware decode, pair mode, the quad
# launch beside the chain (the headline: 163 + 192 workgroups) - and its three batch sizes without spectral norm
SHAPES = [(16, (18, 6), 256, True), (48, (18, 6), 256, True), (48, (16, 6), 256, True), (48, (18, 6), 64, True), (128, (18, 6), 256, True), (256, (18, 6), 256, True),
          (16, (18, 6), 256, False), (48, (18, 6), 256, False), (256, (18, 6), 256, False)]


@pytest.mark.parametrize('B,dims,H,spectral_norm', SHAPES)
def test_six_updates_leave_the_bits_of_the_stream_dependency_schedule_on_the_emulated_kernels(monkeypatch, B, dims, H, spectral_norm):
  tgp = E._emulated_product(monkeypatch, streams=True)
  G.legs_equal_the_control(tgp, monkeypatch, B, dims, H, spectral_norm)


@pytest.mark.parametrize('B,given_eps', G.ORACLE_CASES)
def test_six_headline_updates_replay_through_the_oracle_on_the_emulated_kernels(monkeypatch, B, given_eps):
  tgp = E._emulated_product(monkeypatch, streams=True)
  tt, bench = E._timed_path_modules(monkeypatch, tgp)
  G.headline_updates_against_the_oracle(tt, bench, monkeypatch, given_eps, B)


def test_six_direct_updates_digest_on_the_emulated_kernels(monkeypatch):
  """Six updates (two run(), four launch_direct()) at B = IL_CHAIN_LEGS_EMU_B (48); with IL_CHAIN_LEGS_EMU_DIGEST set the digest of the learner is written there (the
  comparisons below)."""
  tgp = E._emulated_product(monkeypatch, streams=True)
  _, final = G.six_updates(tgp, monkeypatch, int(os.environ.get('IL_CHAIN_LEGS_EMU_B', '48')), (18, 6), 256, True, 'direct', os.environ.get('IL_STAGE_ROWS', '1'))
  h = hashlib.sha256()
  for a in final:
    assert np.isfinite(a).all()
    h.update(np.ascontiguousarray(a).tobytes())
  out = os.environ.get('IL_CHAIN_LEGS_EMU_DIGEST')
  if out:
    with open(out, 'w') as f: json.dump(dict(digest=h.hexdigest()), f)


def _digest(tmp_path, name, **env):
  out = str(tmp_path / f'{name}.json')
  r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider', os.path.abspath(__file__) + '::test_six_direct_updates_digest_on_the_emulated_kernels'],
                     env=dict(os.environ, IL_CHAIN_LEGS_EMU_DIGEST=out, **env), cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=900)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
  with open(out) as f: return json.load(f)['digest']


@pytest.mark.parametrize('B', [48, 256])
def test_schedule_orders_and_draw_orders_are_bit_identical_on_the_emulated_kernels(tmp_path, B):
  """The default order, the reversed schedule, and the late draw (IL_EARLY_DRAW=0: the chain launch is resident before the indices exist, its poll loop spins) under both; with the
  late draw also the rows through the indices (IL_STAGE_ROWS=0): a row index requested ahead of the wait reads the previous draw there."""
  got = {name: _digest(tmp_path, name, IL_CHAIN_LEGS_EMU_B=str(B), **env) for name, env in (
      ('default', {}), ('reverse', dict(IL_EMU_SCHEDULE='reverse')), ('late', dict(IL_EARLY_DRAW='0')), ('late_reverse', dict(IL_EARLY_DRAW='0', IL_EMU_SCHEDULE='reverse')),
      ('indices_late', dict(IL_EARLY_DRAW='0', IL_STAGE_ROWS='0')), ('indices_late_reverse', dict(IL_EARLY_DRAW='0', IL_STAGE_ROWS='0', IL_EMU_SCHEDULE='reverse')))}
  assert len(set(got.values())) == 1, got
