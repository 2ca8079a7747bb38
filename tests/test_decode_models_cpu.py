"""Python models of workgroup re-labellings of the HIP kernels (no GPU): what must hold for ANY launch shape is a bijection plus an ordering property the
device-side waits rely on. The formulas are restated from the kernels (imitation-learning_amd/csrc/mlp_tile.hpp pop_ids, csrc/sac.hip dw_block_job); the -m gpu
tests check the kernels themselves bit for bit."""
import pytest


def pop_ids(bx, by, nx, L):
  """Population launches, grid (nx workgroups per learner, L learners), dispatched in linear order g = by * nx + bx round-robin over 8 XCDs: learner l -> XCD l % 8."""
  g, full = by * nx + bx, (L >> 3) * 8 * nx
  if g < full:
    grp, r = divmod(g, 8 * nx)
    return r >> 3, grp * 8 + (r & 7)
  return bx, by


@pytest.mark.parametrize('nx,L', [(32, 8), (32, 18), (96, 64), (41, 16), (7, 9), (33, 3), (64, 1)])
def test_pop_ids_is_a_bijection_that_pins_a_learner_to_one_xcd_and_keeps_its_block_order(nx, L):
  seen, last_bx = set(), {}
  for g in range(nx * L):          # dispatch order
    by, bx = divmod(g, nx)
    nbx, nby = pop_ids(bx, by, nx, L)
    assert 0 <= nbx < nx and 0 <= nby < L and (nbx, nby) not in seen
    seen.add((nbx, nby))
    if nby < (L >> 3) * 8:
      assert g % 8 == nby % 8, 'a learner of a full group of 8 lives on XCD learner % 8'
    assert last_bx.get(nby, -1) < nbx, "a learner's workgroups are dispatched in increasing block order (a role only waits for lower-numbered workgroups of its learner)"
    last_bx[nby] = nbx
  assert len(seen) == nx * L


@pytest.mark.parametrize('nt,helpers', [(16, 4), (5, 4), (16, 6)])
def test_policy_critic_xcd_decode(nt, helpers):
  crit, help_ = {}, {}
  for bx in range(8 * nt):
    x, q = bx & 7, bx >> 3
    if x >= 2 + helpers: continue
    if x < 2: crit[(x, q)] = bx
    else:
      h = (x - 2) * nt + q
      tile, part = h % nt, h // nt
      assert tile == q and part == x - 2 and (tile, part) not in help_
      help_[(tile, part)] = bx
  assert len(crit) == 2 * nt and len(help_) == helpers * nt
  for (tile, part), bx in help_.items():
    assert crit[(0, tile)] < bx and crit[(1, tile)] < bx, 'a helper only waits for lower-numbered workgroups (both critics of its tile)'


def test_dw_block_xcd_rectangles():
  """csrc/sac.hip dw_block_job: the 64 blocks of an H = 256 layer's dW re-labelled so that XCD x (= workgroup index % 8; a network's job list starts at a
  multiple of 8) owns the 2 x 4 rectangle n in {2 (x / 2), + 1}, k in {4 (x % 2) .. + 3}: a bijection, 2 + 4 operand panels per XCD instead of 8 + 1."""
  seen, panels = set(), {x: (set(), set()) for x in range(8)}
  for job in range(64):
    x, slot = job & 7, job >> 3
    nb, kb = 2 * (x >> 1) + (slot >> 2), 4 * (x & 1) + (slot & 3)
    seen.add((nb, kb))
    panels[x][0].add(nb); panels[x][1].add(kb)
  assert len(seen) == 64 and seen == {(n, k) for n in range(8) for k in range(8)}
  assert all(len(dz) == 2 and len(xp) == 4 for dz, xp in panels.values())
  # the job counts the host and the kernel agree on (dw_block_jobs): per network nbh^2 + nbh * ceil(IN / 32) + ceil(OUT / 32) * nbh, a multiple of 8 at H = 256
  jobs = lambda IN, H, OUT: (H // 32) ** 2 + (H // 32) * ((IN + 31) // 32) + ((OUT + 31) // 32) * (H // 32)
  assert jobs(24, 256, 1) == 80 and jobs(18, 256, 12) == 80 and jobs(120, 256, 1) % 8 == 0


def test_pwil_wave_ranking_equals_full_rank_counting():
  import numpy as np
  """csrc/pwil.hip pw_rank256: a key's rank among the 256 (distance, index) keys of a chunk = its rank inside its wave of 64 + per other wave the number of smaller keys
  found by a branch-free binary search (steps 64 .. 1) over that wave's sorted run padded to 128 slots with the largest key. Must equal counting every key - ties on the
  distance (consumed atoms all carry FLT_MAX), exhausted lists and pad keys included."""
  rng = np.random.RandomState(5)
  for case in range(6):
    dist = rng.uniform(0, 4, 256).astype(np.float32)
    if case >= 1: dist[rng.choice(256, 90, replace=False)] = np.finfo(np.float32).max   # consumed atoms / rows past the end of the set
    if case >= 2: dist[rng.choice(256, 40, replace=False)] = dist[3]                      # exact ties: the index decides
    if case == 5: dist[:] = 1.5
    key = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(256, dtype=np.uint64)
    want = np.array([(key < k).sum() for k in key])
    runs = [np.concatenate([np.sort(key[64 * w:64 * w + 64]), np.full(64, np.uint64(2 ** 64 - 1))]) for w in range(4)]
    got = np.empty(256, np.int64)
    for t in range(256):
      w = t // 64
      r = int((key[64 * w:64 * w + 64] < key[t]).sum())   # the v_readlane loop of the wave
      for q in (1, 2, 3):
        a, pos = runs[(w + q) & 3], 0
        for step in (64, 32, 16, 8, 4, 2, 1):
          if a[pos + step - 1] < key[t]: pos += step
        r += pos
      got[t] = r
    np.testing.assert_array_equal(got, want)
    assert sorted(got) == list(range(256))
