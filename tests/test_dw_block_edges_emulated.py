"""The bodies of tests/test_dw_block_edges_gpu.py - the 32 x 32 block jobs of the optimiser launches and the actor launch's tail at every block kind, one chunk / one trip /
two trips, with the learner's poison word attached, raised and cleared - on the host emulation of the kernels (tests/host_emu), with the parametrisation the GPU module
itself declares (tests/emulated_cases.py) and the GPU's bounds. This is where the seeds are checked against close_params' caps before any GPU visit. What the emulator
can say here: the indexing of every block kind, the arithmetic, that a raised word keeps every store back and that the update is closed all the same; the order of the
memory requests is a property of the compiled code (profiles/dw_one_trip_isa.txt)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import emulated_cases  # noqa: E402
import test_kernels_host_emulation as E  # noqa: E402
import test_dw_block_edges_gpu as G  # noqa: E402


@pytest.mark.parametrize('body,kw', emulated_cases.cases(G))
def test_dw_block_edge_bodies_on_the_emulated_kernels(monkeypatch, tmp_path, body, kw):
  emulated_cases.run(E, G, monkeypatch, tmp_path, body, kw)
