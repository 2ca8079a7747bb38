"""The bodies of tests/test_spec_rows_gpu.py on the host emulation of the kernels (tests/host_emu): the sampler workgroup's private slab, actor(s')'s early request and
its second request behind the wait, the tail's [IL_SYNC_DRAW_SEEN] store and the vouched launch driven by a host store, as co-resident fibers. The emulator's caller
stream is synchronous - the previous update has ended before the next one is enqueued, and the side branch runs beside the main one - so which launches find their draw
vouched for in run() / launch_direct() is whatever its schedule gives; the bits must not depend on it. What it cannot show: a load served from a cache (the GPU file's
IL_EARLY_DRAW=0 case is the one with rows that really are stale)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
import test_spec_rows_gpu as G  # noqa: E402

# one tile and three tiles in pair mode, k_sac_chain behind the new tail word; the other widths and the larger batches run on the GPU (and, for the rest of the chain
# launch, in tests/test_chain_legs_emulated.py, whose staged modes go through the same early request)
SHAPES = [(16, (18, 6), 256), (48, (18, 6), 256), (48, (17, 6), 256), (48, (18, 6), 64)]


@pytest.mark.parametrize('B,dims,H', SHAPES)
def test_eight_updates_leave_the_bits_of_the_stream_dependency_schedule_on_the_emulated_kernels(monkeypatch, B, dims, H):
  tgp = E._emulated_product(monkeypatch, streams=True)
  G.bits_equal_the_control(tgp, monkeypatch, B, dims, H, modes=('run', 'direct'))


@pytest.mark.parametrize('B', [16, 48])
def test_vouched_launch_uses_the_rows_requested_ahead_of_the_wait_on_the_emulated_kernels(monkeypatch, B):
  tgp = E._emulated_product(monkeypatch, streams=True)
  G.vouched_path_is_taken_and_leaves_the_bits(tgp, monkeypatch, B)


@pytest.mark.parametrize('B', [16, 48])
@pytest.mark.parametrize('absorbing', [True, False])
def test_private_slab_holds_next_states_and_absorbing_on_the_emulated_kernels(monkeypatch, B, absorbing):
  tgp = E._emulated_product(monkeypatch, streams=True)
  G.slab_holds_the_drawn_rows(tgp, monkeypatch, B, absorbing)
