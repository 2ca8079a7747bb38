"""The bodies of tests/test_qpass_gpu.py on the host emulation of the kernels (tests/host_emu): the quad critics' mask written at the hop with Q summed beside the
backward, and the helpers' count-and-reset by a thread of the last wave, as co-resident fibers. IL_PAIR, IL_QUAD and IL_EMU_SCHEDULE are read once per process: the
16-wave control, the pair-launch runs and the perturbed schedules go through a subprocess of this file, as in tests/test_tail_loads_emulated.py.

The schedules are what the new concurrency is exposed to: between the receive's barrier and the next, waves 4 .. 7 of quarter 0 read H2s while waves 0 .. 3 read DZ2s and
overwrite H1s, and a helper's count arrives whenever its last wave gets to it. Under IL_EMU_SCHEDULE=reverse the last wave runs FIRST between two barriers (the count is
made, and by the last helper the counter cleared, before any head thread has read what the critics wrote), and the Q waves run ahead of the MFMA waves; random:<seed>
shuffles waves, lanes, workgroups and streams. The digests must be those of the stream-dependency control under the forward schedule.
What the emulator cannot show is time - that is read from the ISA (profiles/qpass_isa.txt) and measured (profiles/qpass.txt)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
import test_chain_legs_gpu as G  # noqa: E402
import test_tail_loads_gpu as T  # noqa: E402
import test_qpass_gpu as Q  # noqa: E402

SCHEDULES = ('reverse', 'random:5')
SCHEDULE_CASES = [(16, (18, 6)), (48, (16, 8))]


def test_six_updates_digests_on_the_emulated_kernels(monkeypatch):
  """Six updates per mode of IL_QPASS_EMU_MODES at B = IL_QPASS_EMU_B, dims IL_QPASS_EMU_DIMS, the critics of IL_QPASS_EMU_EDGE if set; with IL_QPASS_EMU_OUT set the
  digests are written there (the subprocesses below)."""
  tgp = E._emulated_product(monkeypatch, streams=True)
  B, dims = int(os.environ.get('IL_QPASS_EMU_B', '16')), tuple(int(x) for x in os.environ.get('IL_QPASS_EMU_DIMS', '18,6').split(','))
  if os.environ.get('IL_QPASS_EMU_EDGE'): Q.install_edge(monkeypatch, tgp, os.environ['IL_QPASS_EMU_EDGE'])
  out = {mode: T.digests(*G.six_updates(tgp, monkeypatch, B, dims, 256, True, mode)) for mode in os.environ.get('IL_QPASS_EMU_MODES', 'run').split(',')}
  if os.environ.get('IL_QPASS_EMU_OUT'):
    with open(os.environ['IL_QPASS_EMU_OUT'], 'w') as f: json.dump(out, f)


def _fresh_process(tmp_path, edge=''):
  def run(B, dims, modes, **env):
    out = str(tmp_path / ('digests_%d_%s_%s.json' % (B, '_'.join(map(str, dims)), '_'.join(f'{k}{v}'.replace(':', '') for k, v in sorted(env.items())))))
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider', os.path.abspath(__file__) + '::test_six_updates_digests_on_the_emulated_kernels'],
                       env=dict(os.environ, IL_QPASS_EMU_B=str(B), IL_QPASS_EMU_DIMS=','.join(map(str, dims)), IL_QPASS_EMU_MODES=','.join(modes), IL_QPASS_EMU_OUT=out, IL_QPASS_EMU_EDGE=edge, **env),
                       cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    with open(out) as f: return json.load(f)
  return run


@pytest.mark.parametrize('B,dims', Q.CASES)
def test_six_updates_leave_the_bits_of_both_controls_on_the_emulated_kernels(monkeypatch, tmp_path, B, dims):
  tgp = E._emulated_product(monkeypatch, streams=True)
  run = _fresh_process(tmp_path)
  T.bits_equal_both_controls(tgp, monkeypatch, B, dims, other_control=lambda B, dims: run(B, dims, ('run',), IL_PAIR='0')['run'])


@pytest.mark.parametrize('B,dims', Q.PAIR_LAUNCH_CASES)
def test_helpers_of_the_pair_launch_leave_the_bits_of_both_controls_on_the_emulated_kernels(monkeypatch, tmp_path, B, dims):
  tgp = E._emulated_product(monkeypatch, streams=True)
  run = _fresh_process(tmp_path)
  T.pair_launch_equals_both_controls(tgp, monkeypatch, B, dims, run, other_control=lambda B, dims: run(B, dims, ('run',), IL_PAIR='0')['run'])


@pytest.mark.parametrize('edge', Q.EDGES)
def test_value_edges_leave_the_bits_of_both_controls_on_the_emulated_kernels(monkeypatch, tmp_path, edge):
  tgp = E._emulated_product(monkeypatch, streams=True)
  Q.edge_equals_both_controls(tgp, monkeypatch, edge, run=_fresh_process(tmp_path, edge))


@pytest.mark.parametrize('schedule', SCHEDULES)
@pytest.mark.parametrize('B,dims', SCHEDULE_CASES)
def test_perturbed_schedules_leave_the_bits_of_the_control(monkeypatch, tmp_path, B, dims, schedule):
  """Quad launch under every mode, and the pair launch's helpers (IL_QUAD=0), with the waves, workgroups and streams re-ordered."""
  tgp = E._emulated_product(monkeypatch, streams=True)
  run = _fresh_process(tmp_path)
  want = T.digests(*G.six_updates(tgp, monkeypatch, B, dims, 256, True, 'control'))
  for env in ({}, {'IL_QUAD': '0'}):
    got = run(B, dims, T.MODES, IL_EMU_SCHEDULE=schedule, **env)
    for mode in T.MODES:
      T.compare_digests(want, got[mode], f'{schedule}, {env}, {mode}, B {B}, dims {dims}', per_update=mode != 'burst')


def test_six_updates_replay_through_the_oracle_on_the_emulated_kernels(monkeypatch):
  tgp = E._emulated_product(monkeypatch, streams=True)
  tt, bench = E._timed_path_modules(monkeypatch, tgp)
  T.width_replays_through_the_oracle(tt, bench, monkeypatch, Q.ORACLE_DIMS)
