"""The bodies of tests/test_size_edges_gpu.py - every kernel family against its oracle at the batch sizes and hidden widths of tests/golden/inputs.py EDGE_BATCHES /
EDGE_HIDDEN_* - on the host emulation of the kernels (tests/host_emu), with the parametrisation the GPU module itself declares (tests/emulated_cases.py) and the GPU's
bounds. What the emulator can say about a size: the indexing, the ragged tails of the row tiles and row groups, the arithmetic. Alignment and the memory system need the
GPU.
The seed sweep at `training.batch_size=100` runs beside the other emulated sweeps (tests/test_population_acting_emulated.py)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import emulated_cases  # noqa: E402
import test_kernels_host_emulation as E  # noqa: E402
import test_size_edges_gpu as G  # noqa: E402

# The one cell left to the GPU: hidden 257 at depth 8 (7 s of emulated MFMAs). The other heavy cell, B = 384, runs here at depth 8 (hidden 33), and hidden 257 at depths 1 .. 4.
GPU_ONLY = {'general_sac_update_at_edge_sizes-B17-H257-d8-relu-S11A3'}


class _Event:   # torch.cuda.Event (PretrainPlan records one behind every staged copy): the emulated null stream runs every copy at once
  def record(self, *a, **k): pass
  def synchronize(self): pass


@pytest.mark.parametrize('body,kw', [c for c in emulated_cases.cases(G) if c.id not in GPU_ONLY])
def test_size_edge_bodies_on_the_emulated_kernels(monkeypatch, tmp_path, body, kw):
  import torch
  monkeypatch.setattr(torch.cuda, 'Event', _Event)
  emulated_cases.run(E, G, monkeypatch, tmp_path, body, kw)
