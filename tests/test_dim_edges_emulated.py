"""The bodies of tests/test_dim_edges_gpu.py - every kernel family against its oracle at the state / action widths of tests/golden/inputs.py EDGE_DIMS - on the host
emulation of the kernels (tests/host_emu), with the parametrisation the GPU module itself declares (its pytest.mark.parametrize marks are read, not restated:
tests/emulated_cases.py) and the GPU's bounds. What the emulator can say about a width: the indexing, the tile padding, the row layout, the arithmetic. Alignment and
the memory system need the GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import emulated_cases  # noqa: E402
import test_kernels_host_emulation as E  # noqa: E402
import test_dim_edges_gpu as G  # noqa: E402


@pytest.mark.parametrize('body,kw', emulated_cases.cases(G))
def test_dim_edge_bodies_on_the_emulated_kernels(monkeypatch, tmp_path, body, kw):
  emulated_cases.run(E, G, monkeypatch, tmp_path, body, kw)
