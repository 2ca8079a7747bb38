"""The bodies of tests/test_value_edges_gpu.py - every kernel family against its oracle at the values where the kernels branch: clamps, saturation, ties, zero weights -
on the host emulation of the kernels (tests/host_emu), with the parametrisation the GPU module itself declares (tests/emulated_cases.py) and the GPU's bounds. What the
emulator can say about a value: which branch a kernel takes and what it computes there with the host's libm. What the device's own tanhf / atanhf / expf / log1pf / logf
return at these arguments, the hardware exp2's denormal flush and ties resolved across real waves need the GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import emulated_cases  # noqa: E402
import test_kernels_host_emulation as E  # noqa: E402
import test_value_edges_gpu as G  # noqa: E402

GPU_ONLY = set()


class _Event:   # torch.cuda.Event: the emulated null stream runs every copy at once
  def record(self, *a, **k): pass
  def synchronize(self): pass


@pytest.mark.parametrize('body,kw', [c for c in emulated_cases.cases(G) if c.id not in GPU_ONLY])
def test_value_edge_bodies_on_the_emulated_kernels(monkeypatch, tmp_path, body, kw):
  import torch
  monkeypatch.setattr(torch.cuda, 'Event', _Event)
  emulated_cases.run(E, G, monkeypatch, tmp_path, body, kw)
