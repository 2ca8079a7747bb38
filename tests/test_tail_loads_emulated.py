"""The bodies of tests/test_tail_loads_gpu.py on the host emulation of the kernels (tests/host_emu): the helpers' prefetched W3 / h2 lanes and
the targets' first layer in two parts around the wait for a', as co-resident fibers. IL_PAIR and IL_QUAD are read once per process: the 16-wave control and the
pair-launch runs go through a subprocess of this file, as tests/test_chain_legs_emulated.py does for its switches. What the emulator cannot show is time - that a
request now travels ahead of its barrier is read from the ISA (profiles/tail_loads_isa.txt) and measured (profiles/tail_loads.txt)."""
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

# every width at three tiles, the headline width at one tile and at eight (the larger shapes of the GPU file's other widths run there)
CASES = [(48, w) for w in T.WIDTHS] + [(16, (18, 6)), (128, (18, 6))]


def test_six_updates_digests_on_the_emulated_kernels(monkeypatch):
  """Six updates per mode of IL_TAIL_EMU_MODES at B = IL_TAIL_EMU_B, dims IL_TAIL_EMU_DIMS; with IL_TAIL_EMU_OUT set the digests are written there (the subprocesses below)."""
  tgp = E._emulated_product(monkeypatch, streams=True)
  B, dims = int(os.environ.get('IL_TAIL_EMU_B', '16')), tuple(int(x) for x in os.environ.get('IL_TAIL_EMU_DIMS', '18,6').split(','))
  out = {mode: T.digests(*G.six_updates(tgp, monkeypatch, B, dims, 256, True, mode)) for mode in os.environ.get('IL_TAIL_EMU_MODES', 'run').split(',')}
  if os.environ.get('IL_TAIL_EMU_OUT'):
    with open(os.environ['IL_TAIL_EMU_OUT'], 'w') as f: json.dump(out, f)


def _fresh_process(tmp_path):
  def run(B, dims, modes, **env):
    out = str(tmp_path / ('digests_%d_%s_%s.json' % (B, '_'.join(map(str, dims)), '_'.join(f'{k}{v}' for k, v in sorted(env.items())))))
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider', os.path.abspath(__file__) + '::test_six_updates_digests_on_the_emulated_kernels'],
                       env=dict(os.environ, IL_TAIL_EMU_B=str(B), IL_TAIL_EMU_DIMS=','.join(map(str, dims)), IL_TAIL_EMU_MODES=','.join(modes), IL_TAIL_EMU_OUT=out, **env),
                       cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    with open(out) as f: return json.load(f)
  return run


@pytest.mark.parametrize('B,dims', CASES)
def test_six_updates_leave_the_bits_of_both_controls_on_the_emulated_kernels(monkeypatch, tmp_path, B, dims):
  tgp = E._emulated_product(monkeypatch, streams=True)
  run = _fresh_process(tmp_path)
  T.bits_equal_both_controls(tgp, monkeypatch, B, dims, other_control=lambda B, dims: run(B, dims, ('run',), IL_PAIR='0')['run'])


@pytest.mark.parametrize('B,dims', T.PAIR_LAUNCH_CASES)
def test_helpers_of_the_pair_launch_leave_the_bits_of_both_controls_on_the_emulated_kernels(monkeypatch, tmp_path, B, dims):
  tgp = E._emulated_product(monkeypatch, streams=True)
  run = _fresh_process(tmp_path)
  T.pair_launch_equals_both_controls(tgp, monkeypatch, B, dims, run, other_control=lambda B, dims: run(B, dims, ('run',), IL_PAIR='0')['run'])


@pytest.mark.parametrize('dims', T.WIDTHS)
def test_six_updates_replay_through_the_oracle_at_every_width_on_the_emulated_kernels(monkeypatch, dims):
  tgp = E._emulated_product(monkeypatch, streams=True)
  tt, bench = E._timed_path_modules(monkeypatch, tgp)
  T.width_replays_through_the_oracle(tt, bench, monkeypatch, dims)
