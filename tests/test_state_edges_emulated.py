"""The bodies of tests/test_state_edges_gpu.py - the state that the replay and acting kernels carry from one launch to the next, at the points where it wraps - on the host
emulation of the kernels (tests/host_emu), with the parametrisation the GPU module itself declares (tests/emulated_cases.py). What the emulator can say about a wrap
point: the index arithmetic, the order of the stores behind a barrier (its lanes do not run in lockstep), the stream compaction. The mailbox in pinned memory, the
system-scope release of the echo and the memory system need the GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import emulated_cases  # noqa: E402
import test_kernels_host_emulation as E  # noqa: E402
import test_state_edges_gpu as G  # noqa: E402


@pytest.mark.parametrize('body,kw', emulated_cases.cases(G))
def test_state_edge_bodies_on_the_emulated_kernels(monkeypatch, tmp_path, body, kw):
  emulated_cases.run(E, G, monkeypatch, tmp_path, body, kw)
