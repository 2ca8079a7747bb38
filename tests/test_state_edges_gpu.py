"""`-m gpu`: the state that the replay and acting kernels carry from one launch to the next, at the points where it WRAPS. The sibling modules cover the shapes
(tests/test_dim_edges_gpu.py, tests/test_size_edges_gpu.py) and the values (tests/test_value_edges_gpu.py); a run passes the points below all the time, and the rest of the suite
meets them by accident of a seed. Everything device-side is reached through the names of tests/test_gpu_parity.py (`P.il`, `P.T`, ...), which
tests/test_state_edges_emulated.py rebinds to the host emulation of the kernels. Parts 1 to 3 compare bit for bit (integers, copied floats, -0.0 through an int32 view): no
tolerance is introduced; part 4 runs a sibling body under the sibling's bounds.

Wrap points, where they are, and the case that drives each:
  ring cursor: memory.py `_advance`; `ring_state[0] = nc % p.cap`, `if (nc >= p.cap) ring_state[1] = 1` act_mail.hpp:89-90 (act_commit); `(cursor + r) % capacity`
    replay.hip:39 (k_write_rows)                       test_acting_worker_*, test_population_acting_*, test_write_rows_behind_the_grid_cap_across_the_ring_end
  absorbing wrap, a two-row append: `ring[((p.cursor + 1) % p.cap) * row + c]` act_mail.hpp:76 (act_append: the pair straddles the ring end when the episode ends in slot
    cap - 1), `adv = 2` with nc == cap act_mail.hpp:88 (it ends in slot cap - 2: the pair fills the ring, and sets `full`), k_wrap_absorbing replay.hip:52 on the
    per-function side                                  the same cases: _ring_end_script puts true terminations into slot 2, slot cap - 2 and slot cap - 1, in that order
  commit word: sequence * 64 + flags as fp32, `_seq % (_SEQ_MOD - 1) + 1` acting.py:44, 188, 405, 409: from 131071 to 1; act_pending / `uncoupled` compare words
    act_mail.hpp:33, 52; act_carry_coupled act_mail.hpp:28, written by k_pwil_couple (pwil.hip)
                                                       every [seqwrap] case: `_seq` (and `_eval_seq`) start at _SEQ_MOD - 6
  MT19937 device draw, mt_device.hpp: the excluded slot `((idx - 1) % size + size) % size` :39; the degenerate range :44; the prepared block :51 and the twist in place
    :57; the partial chunk in front of a block boundary `take = avail < 256 ? avail : 256` :75; `sh.pos = pos + sh.last + 1` :93; k_sample2 / k_sample2_pop / k_gather2 /
    k_gather2_pop replay.hip:261-327                   test_device_draw_*, test_two_ring_sample_*, test_population_sample_*
  grid-stride loops behind a capped grid: k_gather, k_write_rows (1024 workgroups: replay.hip:29, 46), k_mix_relabel (512: replay.hip:100, 113), k_mix_relabel_population
    with mix_copy_expert's carried column `c += dc` (512: replay.hip:138-144, 183), k_g_pack_sac (256: general.hip:1009; the (s, a) matrix alone crosses it)
                                                       test_*_behind_the_grid_cap*, test_general_sac_update_behind_the_pack_cap

Conditions on the INPUTS, asserted on the reference's side (EdgeNotMet) so that a change of seeds cannot empty a case without notice:
  (a) one call consumes 2 x 624 words or more and crosses two block boundaries (n = 1000 at 513 rows): the prepared block AND the twist in place;
  (b) one call finds the generator at 624 and leaves it at exactly 624 (n = 624, a full ring of 1024 rows, the excluded slot does not come up), the next call is n = 1;
  (c) the excluded slot is size - 1 (idx = 0) in one state and 0 (idx = 1) in another, and for rings of up to 257 rows the reference met and rejected it;
  (d) a batch ends in the last lane of a 256-chunk, and one in the last lane of the partial chunk in front of a block boundary (_trips restates the chunking);
  (e) every call consumes at most WORDS_BOUND = 4200 words, i.e. at most 4201 trips of mt_draw's loop, whose guard is 100000;
  the degenerate range consumes no word; oracle/mt19937.py is itself pinned, in every call, to the literal loop of the reference's memory.py:51-56 on np.random.RandomState;
  acting: the oracle ring's cursor in front of every true termination is the slot the script is built for, the ring wraps, `_seq` ends below where it started, the
  overlap schedule's replayed launch fell on the post that wrapped the sequence (and on every true termination, the straddling one among them), the learners differ.
Not full with idx in {0, 1}: the reference raises, the host draw refuses, the device draw would write zeros: ReplayMemory.sample_device now refuses on the host in the host
draw's words (test_sample_device_refuses_a_ring_without_a_slot_to_draw). No existing test relied on the zeros.

Seeds (SEEDS): fixed bases. Rejected, on the reference alone: boundary 5300 (the excluded slot comes up at word 960 of the 1136 the case needs free of it; likewise 5302 - 5305:
words 710, 548, 442, 464); 5301 in use. No seed was rejected for a comparison.

Found by this module: nothing - every case passes on the emulated kernels and on the MI355X.

Broken on purpose once, in a scratch copy, on the emulated kernels only (each line: the cases that then fail; every mutation stays inside its buffers):
  act_commit `nc >= p.cap` -> `>`: every case of acting_worker (56) and pwil_coupling (18), population_acting (12) and pwil_population_coupling (12): the device ring state behind the
    append that fills the ring. `full` is sticky - at the end of a run a later append has long set it - so the ring state is checked behind EVERY append, and the script ends
    its episodes in slot cap - 2 before slot cap - 1: the pair that fills the ring exactly is then also the first to set `full`
  act_commit `nc % p.cap` -> `(p.cursor + 1) % p.cap`: every absorbing case of acting_worker (48), population_acting (12), pwil_coupling (18), pwil_population_coupling (12)
  act_append, the absorbing row written to `p.cursor` again where it would wrap: every absorbing case of the four acting bodies (48, 12, 18, 12). Later appends
    overwrite both slots of a pair (the populations' scripts run two laps), so the whole ring is compared behind EVERY step, with the reference's and with the oracle's
  mt_draw `excl` without `+ size`: device_draw_at_full_ring_states[2 .. 1025] (28: idx = 0 gives -1, slot size - 1 is drawn), device_draw_crosses_two_blocks_in_one_call,
    two_ring_sample[pow2-idx0+notfull-257], [513-idx0+5-last], population_sample_at_differing_ring_states (the three sizes from 1e6 up pass: slot size - 1 does not come up)
  mt_draw `sh.pos = pos + sh.last + 1` -> `pos + take`: all 31 device_draw_at_full_ring_states, device_draw_at_not_full_ring_states, crosses_two_blocks, ends_on_the_block_boundary,
    all four two_ring_sample, population_sample
  mt_draw without the copy of the prepared block: the same 38 without population_sample (k_sample2_pop prepares no block)
  mt_draw without its degenerate branch: device_draw_at_not_full_ring_states, two_ring_sample[degenerate+33-idx2], population_sample_at_differing_ring_states (zeros all
    the same, n words consumed: the next call shows it)
  mix_copy_expert `dc` -> 0: mix_relabel_launches_behind_the_grid_cap[label1-SQIL], [label2-AdRIL], mix_relabel_population_behind_the_grid_cap_off_the_16_byte_grid (label 0
    patches no reward column: it passes, as it must)
  k_write_rows without cursor and `% capacity` (`ring[r * row + c]`: in bounds while n <= capacity): both write_rows_behind_the_grid_cap_across_the_ring_end, every
    acting_worker (56) and pwil_coupling (18) case (the per-function append)

Largest measured deviation over its bound in part 4: RECORDS below. Run time of the module: 6 s on the MI355X (154 cases, the slowest 0.4 s); the emulated module takes
about 40 s."""
import atexit
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import inputs as gi
import test_gpu_parity as P
import test_size_edges_gpu as Z
from oracle import adril as oadril
from oracle import replay as oreplay
from oracle.mt19937 import MT19937, sample_indices

pytestmark = pytest.mark.gpu

SEQ_MOD = 1 << 17                      # imitation_learning_amd/acting.py _SEQ_MOD (asserted against it where a worker is built)
SEEDS = dict(draw=5000, not_full=5100, two_blocks=5201, boundary=5301, two_rings=5400, population=5500, acting=5, mix=5600, rows=5700, sac=5800)
GUARD, SENTINEL = 32, -7.5             # guard floats (a whole number of 16-byte lanes) on both sides of a row buffer; guard ints behind an index array hold -1

# family -> largest measured deviation over its bound, (emulated kernels, MI355X): part 4 alone has a bound; everything else in this module is compared bit for bit
RECORDS = {
    'general SAC': (0.21, 0.12),
    'general SAC (parameters)': (5.3e-05, 9.5e-05),
}

WORST = {}   # this run's figures, written to $IL_STATE_EDGES_RECORD as JSON when the process ends


@atexit.register
def _write_records():
  if os.environ.get('IL_STATE_EDGES_RECORD') and WORST:
    with open(os.environ['IL_STATE_EDGES_RECORD'], 'w') as f: json.dump(WORST, f, indent=1, sort_keys=True)


@contextlib.contextmanager
def _recording():
  saved, Z.WORST = Z.WORST, WORST
  try: yield
  finally: Z.WORST = saved


class EdgeNotMet(AssertionError):
  """A condition on the INPUTS, checked on the reference's side: the case no longer passes the wrap point it is about."""


def _met(cond, what):
  if not cond: raise EdgeNotMet(what)


def _bits(a):
  return np.ascontiguousarray(a).view(np.int32)


def _same_bits(got, want, what):
  np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)   # -0.0 is not 0.0 here


# ================================================================================================ 1. the device index draw
DRAW_NS = (1, 63, 64, 65, 255, 256, 257, 624, 625, 1000)
DRAW_SIZES = tuple(sorted({s for k in range(1, 11) for s in (2 ** k - 1, 2 ** k, 2 ** k + 1) if s >= 2})) + (1_000_000, 2 ** 24 + 1, 2 ** 31 - 1)
NOT_FULL_IDX = (2, 3, 4, 5, 9, 17, 257)
# (e) every trip of mt_draw's loop consumes at least one word of the stream, so a call that consumes w words takes at most w + 1 trips: with w <= WORDS_BOUND a call stays a
# factor of 20 below the guard of 100000 trips. The worst acceptance rate of the states below is 1 / 2 (a 2^k + 1 ring: (2^k + 1) / 2^(k + 1) for the mask, 2^k / (2^k + 1)
# for the excluded slot), i.e. ~2 n words: 4 n + 200 holds them with a margin of some 20 standard deviations at n = 1000
WORDS_BOUND = 4 * max(DRAW_NS) + 200


class _Counting(MT19937):
  words = 0

  def next_uint32(self):
    self.words += 1
    return super().next_uint32()


def _literal_draw(rs, n, size, idx, full):
  """`[memory._sample_idx() for _ in range(n)]`, the loop of the reference's memory.py:51-56 on a np.random.RandomState; and how often the excluded slot came up."""
  out, excluded = [], 0
  for _ in range(n):
    valid_idx = False
    while not valid_idx:
      i = rs.randint(0, size if full else idx - 1)
      valid_idx = i != (idx - 1) % size
      excluded += not valid_idx
    out.append(int(i))
  return out, excluded


def _trips(pos, words):
  """(candidates offered, candidates consumed) per trip of mt_draw for a call that finds the generator at `pos` and consumes `words` words: 256 at a time, fewer in front of
  a block boundary; every trip but the last consumes what it offers."""
  out = []
  while words > 0:
    if pos >= 624: pos = 0
    take = min(256, 624 - pos)
    used = min(take, words)
    out.append((take, used)); pos += used; words -= used
  return out


class _Stream:
  """One generator state three times: oracle/mt19937.py (counting its words), numpy's legacy RandomState, and the 625 words on the device."""

  def __init__(self, seed):
    self.seed, self.gen, self.rs = seed, _Counting(seed), np.random.RandomState(seed)
    self.state = P.il_memory.IndexStream(seed).device_state(P.DEV)
    self.calls = []   # (pos before, words, times the excluded slot came up) per reference call

  def reference(self, n, size, idx, full):
    pos, w0 = self.gen.pos, self.gen.words
    want = sample_indices(self.gen, n, size, idx, full)
    literal, excluded = _literal_draw(self.rs, n, size, idx, full)
    assert want == literal, f'oracle/mt19937.py against numpy: seed {self.seed}, n {n}, size {size}, idx {idx}, full {full}'
    words = self.gen.words - w0
    _met(words <= WORDS_BOUND, f'(e) {words} words in one call of n = {n} (size {size}, idx {idx}): above the bound of {WORDS_BOUND}')
    self.calls.append((pos, words, excluded))
    return np.asarray(want, np.int64)

  def assert_state(self, what):
    got = P.N(self.state).view(np.uint32)
    assert int(got[624]) == self.gen.pos, f'{what}: the generator stands at {int(got[624])}, the reference at {self.gen.pos}'
    np.testing.assert_array_equal(got[:624], np.asarray(self.gen.mt, np.uint32), err_msg=f'{what}: the 624 words')


def _ring_state(idx, full, size):
  return torch.tensor([idx, int(full), size], dtype=torch.int64).to(P.DEV)


def _draw(stream, n, size, idx, full):
  """One il_mt19937_sample_indices_device call (no ring is allocated) against the reference; guard ints behind the n indices."""
  want = stream.reference(n, size, idx, full)
  rs, out = _ring_state(idx, full, size), torch.full((n + GUARD,), -1, dtype=torch.int32).to(P.DEV)
  P._lib.check(P._lib.lib().il_mt19937_sample_indices_device(P._lib.ptr(stream.state), P._lib.ptr(rs), n, P._lib.ptr(out), P._lib.stream_ptr()))
  torch.cuda.synchronize()
  got = P.N(out)
  what = f'seed {stream.seed}, call {len(stream.calls)}: n {n}, size {size}, idx {idx}, full {full}'
  np.testing.assert_array_equal(got[:n].astype(np.int64), want, err_msg=what)
  assert (got[n:] == -1).all(), f'{what}: an index was written behind the n-th'
  return want


def _full_idx(size):
  return sorted({i for i in (0, 1, 2, size - 1) if i < size})


@pytest.mark.parametrize('size', DRAW_SIZES)
def test_device_draw_at_full_ring_states(size):
  """A full ring of `size` rows with the cursor at 0, 1, 2 and size - 1 (the excluded slot (idx - 1) % size is size - 1, 0, 1 and size - 2): every n of DRAW_NS at
  every state, ten calls on one generator state each, the order of the n rotated from state to state. Conditions: (c), (e); the generator's 625 words after the last call."""
  for k, idx in enumerate(_full_idx(size)):
    s = _Stream(SEEDS['draw'] + 4 * DRAW_SIZES.index(size) + k)
    r = (DRAW_SIZES.index(size) + 3 * k) % len(DRAW_NS)
    for n in DRAW_NS[r:] + DRAW_NS[:r]:
      got = _draw(s, n, size, idx, True)
      assert ((idx - 1) % size) not in got and got.min() >= 0 and got.max() < size
    s.assert_state(f'size {size}, idx {idx}')
    if size <= 257:   # (c) 3553 draws: the excluded slot is expected to come up 14 times or more
      _met(sum(c[2] for c in s.calls) > 0, f'(c) the excluded slot {(idx - 1) % size} of a ring of {size} never came up')
  excl = {(i - 1) % size for i in _full_idx(size)}
  _met(size - 1 in excl and 0 in excl, '(c) the excluded slot is meant to be size - 1 in one state and 0 in another')


def test_device_draw_at_not_full_ring_states():
  """Rings that have not wrapped, cursor at 2, 3, 4, 5, 9, 17 and 257 (the draw is from [0, idx - 2]), ONE generator state through all of them, every n of DRAW_NS: idx = 2
  is the degenerate range - zeros, and no word consumed, which the next call (idx = 3, another range) shows on the continuing stream. The ring's size does not enter a
  not-full draw; both sizes of the word `size` are used (1000, 2^31 - 1)."""
  s = _Stream(SEEDS['not_full'])
  for j, n in enumerate(DRAW_NS):
    for idx in NOT_FULL_IDX:
      size = (1000, 2 ** 31 - 1)[j % 2]
      got = _draw(s, n, size, idx, False)
      assert got.max() <= idx - 2
      if idx == 2:
        _met(s.calls[-1][1] == 0, 'the degenerate range is meant to consume no word of the reference stream')
        assert not got.any()
        s.assert_state(f'behind the degenerate range, n {n}')
  s.assert_state('the last call')
  _met(sum(c[1] for c in s.calls) > 6 * sum(DRAW_NS) // 2, 'the other ranges are meant to consume the stream')


def test_device_draw_crosses_two_blocks_in_one_call():
  """(a) n = 1000 at a 2^k + 1 ring (513 rows, full, cursor 0: half of the candidates are rejected) consumes some 2000 words in ONE call: the first block boundary is
  crossed with the block mt_next_block prepared, the second and third with the twist in place (mt_device.hpp:51-74). Three calls of 1000, then 1."""
  s = _Stream(SEEDS['two_blocks'])
  for n in (1000, 1000, 1000, 1):
    _draw(s, n, 513, 0, True)
  crossings = [(pos + words - 1) // 624 if words else 0 for pos, words, _ in s.calls]
  _met(max(c[1] for c in s.calls) >= 2 * 624 and max(crossings) >= 2, f'(a) no call consumed 2 x 624 words and crossed two block boundaries: {s.calls}')
  s.assert_state('after four calls')


BOUNDARY_SEED = SEEDS['boundary']


def test_device_draw_ends_on_the_block_boundary():
  """(b) a freshly seeded generator (position 624), a full ring of 1024 rows (no candidate is rejected by the mask) and n = 624 at a seed where the excluded slot does not
  come up: the call consumes exactly one block and leaves the position at 624 - `sh.pos = pos + sh.last + 1` with the last accepted candidate in the last lane of the
  PARTIAL chunk in front of the block boundary (d); the next call is n = 1. Then n = 255 from position 1 and n = 256 from position 256: the batch ends in the last lane of
  a whole 256-chunk (d)."""
  s = _Stream(BOUNDARY_SEED)
  _draw(s, 624, 1024, 5, True)
  _met(s.calls[-1][:2] == (624, 624) and s.gen.pos == 624, f'(b) the call is meant to consume exactly one block: {s.calls[-1]}')
  _met(_trips(*s.calls[-1][:2])[-1] == (112, 112), '(d) the batch is meant to end in the last lane of the partial chunk')
  s.assert_state('position 624')
  _draw(s, 1, 1024, 5, True)
  _met(s.gen.pos == 1, '(b) the call behind the boundary is meant to take one word of the next block')
  _draw(s, 255, 1024, 5, True)
  _draw(s, 256, 1024, 5, True)
  _met(s.calls[-1][:2] == (256, 256) and _trips(256, 256)[-1] == (256, 256), f'(d) the batch is meant to end in the last lane of a 256-chunk: {s.calls[-1]}')
  s.assert_state('after four calls')


def _filled_ring(cap, S, A, idx, full, seed):
  mem = P.il.ReplayMemory(cap, S, A, True, device=P.DEV)
  mem.ring.copy_(P.T(np.random.RandomState(seed).standard_normal((cap, mem.row)).astype(np.float32)))
  mem.idx, mem.full = idx, full
  mem._sync_ring_state()
  return mem


# (capacity, idx, full) of ring A and of ring B: the states of the draw cases above, two different ones per call
TWO_RING_STATES = [pytest.param((8, 0, True), (1025, 257, False), id='pow2-idx0+notfull-257'), pytest.param((9, 8, True), (64, 1, True), id='9-last+pow2-idx1'),
                   pytest.param((1000, 2, False), (33, 2, True), id='degenerate+33-idx2'), pytest.param((513, 0, True), (5, 4, True), id='513-idx0+5-last')]


@pytest.mark.parametrize('a,b', TWO_RING_STATES)
def test_two_ring_sample_at_differing_ring_states(a, b):
  """il_replay_sample_device: ring A then ring B from one generator state in one launch (k_sample2 with both rings, k_gather2), rows of 20 and of 32 floats, four calls:
  indices against the reference stream, rows against fancy indexing. A degenerate ring A leaves the stream to ring B untouched."""
  ma, mb = _filled_ring(a[0], 5, 2, a[1], a[2], SEEDS['two_rings']), _filled_ring(b[0], 11, 3, b[1], b[2], SEEDS['two_rings'] + 1)
  s = _Stream(SEEDS['two_rings'] + a[0] + b[0])
  ring_a, ring_b = P.N(ma.ring), P.N(mb.ring)
  slots, stride = P._lib.sync_layout()[0], P._lib.sync_layout()[3]
  for n in (65, 1000, 257, 624):
    sync = torch.zeros(slots, dtype=torch.int64).to(P.DEV) if n == 624 else None   # the last call with the il_sync counters: k_gather2 writes its rows through and signals
    want_a, want_b = s.reference(n, ma.size, ma.idx, ma.full), s.reference(n, mb.size, mb.idx, mb.full)
    ia, ib = (torch.full((n + GUARD,), -1, dtype=torch.int32).to(P.DEV) for _ in range(2))
    ra, rb = (torch.full((n * m.row + GUARD,), SENTINEL, dtype=torch.float32).to(P.DEV) for m in (ma, mb))
    p = P._lib.ptr
    P._lib.check(P._lib.lib().il_replay_sample_device(p(s.state), n, p(ma._ring_state), p(ma.ring), ma.size, ma.row, p(ia), p(ra), p(mb._ring_state), p(mb.ring), mb.size, mb.row, p(ib), p(rb),
                                                      p(sync), P._lib.stream_ptr()))
    torch.cuda.synchronize()
    workgroups = -(-(n * (ma.row // 4) + n * (mb.row // 4)) // 256)
    assert P._lib.lib().il_replay_gather_workgroups(n, ma.row, mb.row) == workgroups
    if sync is not None:   # include/il_hip.h: [IL_SYNC_INDICES] (line 8) counts the draws, [IL_SYNC_ROWS] (line 0) the gather workgroups that have their rows in place
      counters = P.N(sync)
      assert counters[8 * stride] == 1 and counters[0] == workgroups and counters.sum() == 1 + workgroups, 'the il_sync counters behind a draw with rows'
    for tag, got_i, got_r, want, ring, m in (('A', P.N(ia), P.N(ra), want_a, ring_a, ma), ('B', P.N(ib), P.N(rb), want_b, ring_b, mb)):
      np.testing.assert_array_equal(got_i[:n].astype(np.int64), want, err_msg=f'ring {tag}, n {n}')
      assert (got_i[n:] == -1).all() and (got_r[n * m.row:] == SENTINEL).all(), f'ring {tag}, n {n}: written behind the batch'
      _same_bits(got_r[:n * m.row].reshape(n, m.row), ring[want], f'rows of ring {tag}, n {n}')
  s.assert_state('after four calls')
  if not a[2] and a[1] == 2: _met(all(c[1] == 0 for c in s.calls[0::2]) and all(c[1] > 0 for c in s.calls[1::2]), 'ring A is meant to be the degenerate range')


def test_population_sample_at_differing_ring_states():
  """il_replay_sample_population (k_sample2_pop: one workgroup per learner, no prepared block - every boundary is the twist in place; k_gather2_pop): four learners with
  their own generator states and pairs of ring states that differ from learner to learner; learner 3 has no second ring. Three calls per n."""
  states = [((8, 0, True), (1025, 257, False)), ((513, 1, True), (1000, 2, False)), ((9, 8, True), (64, 1, True)), ((1025, 2, True), None)]
  learners = []
  for l, (a, b) in enumerate(states):
    ma = _filled_ring(a[0], 5, 2, a[1], a[2], SEEDS['population'] + 2 * l)
    mb = _filled_ring(b[0], 11, 3, b[1], b[2], SEEDS['population'] + 2 * l + 1) if b else None
    learners.append((ma, mb, _Stream(SEEDS['population'] + 10 + l)))
  for n in (1000, 65, 256):
    bufs, args = [], []
    for ma, mb, s in learners:
      ia, ib = (torch.full((n + GUARD,), -1, dtype=torch.int32).to(P.DEV) for _ in range(2))
      ra = torch.full((n * ma.row + GUARD,), SENTINEL, dtype=torch.float32).to(P.DEV)
      rb = torch.full((n * (mb.row if mb else 4) + GUARD,), SENTINEL, dtype=torch.float32).to(P.DEV)
      bufs.append((ia, ra, ib, rb))
      args.append(P._lib.SampleArgs(s.state.data_ptr(), ma._ring_state.data_ptr(), ma.ring.data_ptr(), ma.size, ma.row, ia.data_ptr(), ra.data_ptr(),
                                    mb._ring_state.data_ptr() if mb else None, mb.ring.data_ptr() if mb else None, mb.size if mb else 0, mb.row if mb else 0,
                                    ib.data_ptr() if mb else None, rb.data_ptr() if mb else None))
    dev = P.il_training._device_array(args, P.DEV)
    P._lib.check(P._lib.lib().il_replay_sample_population(P._lib.ptr(dev), len(learners), n, 32, P._lib.stream_ptr()))
    torch.cuda.synchronize()
    for l, ((ma, mb, s), (ia, ra, ib, rb)) in enumerate(zip(learners, bufs)):
      for tag, m, gi_, gr in (('A', ma, P.N(ia), P.N(ra)), ('B', mb, P.N(ib), P.N(rb))):
        if m is None:
          assert (gi_ == -1).all() and (gr == SENTINEL).all(), f'learner {l} has no ring B'
          continue
        want = s.reference(n, m.size, m.idx, m.full)
        np.testing.assert_array_equal(gi_[:n].astype(np.int64), want, err_msg=f'learner {l}, ring {tag}, n {n}')
        assert (gi_[n:] == -1).all() and (gr[n * m.row:] == SENTINEL).all(), f'learner {l}, ring {tag}, n {n}: written behind the batch'
        _same_bits(gr[:n * m.row].reshape(n, m.row), P.N(m.ring)[want], f'rows of learner {l}, ring {tag}, n {n}')
  for l, (_, _, s) in enumerate(learners): s.assert_state(f'learner {l}')
  _met(max(c[1] for c in learners[1][2].calls) >= 2 * 624, 'learner 1 (513 rows) is meant to cross two block boundaries in one call')


@pytest.mark.parametrize('high', [1, 2, 3, 1024, 1025, 2 ** 31 - 1])
def test_host_randint_on_the_index_stream(high):
  """IndexStream.randint (il_mt19937_randint: `np.random.choice(subsample)` of environments.py draws from the stream the index draws use) against numpy's legacy randint,
  700 draws - across a block boundary - followed by an index draw that continues the same stream; high = 1 consumes nothing."""
  stream, rs, gen = P.il_memory.IndexStream(SEEDS['draw'] + high % 97), np.random.RandomState(SEEDS['draw'] + high % 97), _Counting(SEEDS['draw'] + high % 97)
  assert [stream.randint(high) for _ in range(700)] == [int(rs.randint(0, high)) for _ in range(700)] == [gen.randint(high) for _ in range(700)]
  _met((gen.words == 0) == (high == 1) and (high == 1 or gen.words >= 700), 'every range but the degenerate one is meant to cross a block boundary')
  want, _ = _literal_draw(rs, 64, 1000, 10, True)
  assert stream.draw(64, 1000, 10, True).tolist() == want == sample_indices(gen, 64, 1000, 10, True)


@pytest.mark.parametrize('idx,full,size,words', [(0, False, 100, 'empty or oversized range (high=-1)'), (1, False, 100, 'empty or oversized range (high=0)'),
                                                 (0, True, 1, 'the only candidate slot is the excluded one')])
def test_sample_device_refuses_a_ring_without_a_slot_to_draw(idx, full, size, words):
  """A ring that is not full with its cursor at 0 or 1 (the reference raises: np.random.randint(0, idx - 1)), and a full ring of one row: ReplayMemory.sample_device refuses
  in the words of the host draw (tests/test_abi_and_layout.py::test_host_index_draw_rejects_empty_ranges), nothing is launched, the stream stays where it was; the host
  draw refuses the same states; and idx = 2, the first state with a slot, is served."""
  mem = _filled_ring(size, 5, 2, idx, full, 1)
  mem.index_rng = P.il_memory.IndexStream(7)
  before = P.N(mem.index_rng.device_state(P.DEV))
  idx_out, rows_out = torch.full((8,), -1, dtype=torch.int32).to(P.DEV), torch.full((8, mem.row), SENTINEL).to(P.DEV)
  with pytest.raises(RuntimeError, match='il_mt19937_sample_indices_device: ' + words.replace('(', r'\(').replace(')', r'\)')):
    mem.sample_device(8, idx_out, rows_out)
  torch.cuda.synchronize()
  assert (P.N(idx_out) == -1).all() and (P.N(rows_out) == SENTINEL).all()
  np.testing.assert_array_equal(P.N(mem.index_rng.device_state(P.DEV)), before)
  with pytest.raises(RuntimeError, match='il_mt19937_sample_indices: ' + words.split(' (')[0]):
    P.il_memory.IndexStream(7).draw(8, size, idx, full)
  if not full:
    mem.idx = 2; mem._sync_ring_state()
    mem.sample_device(8, idx_out, rows_out)
    torch.cuda.synchronize()
    assert (P.N(idx_out) == 0).all()
    _same_bits(P.N(rows_out), np.repeat(P.N(mem.ring)[:1], 8, axis=0), 'eight times row 0')


# ================================================================================================ 2. acting: ring end and sequence wrap
# name: (S, A, hidden, depth, activation). il_act_step; il_act_step_general as one launch (the tile engine) and as layer-at-a-time launches plus the commit kernel
ACT_SHAPES = {'fused': (18, 6, 64, 2, 'relu'), 'general_one_launch': (12, 3, 48, 3, 'tanh'), 'general_layers': (12, 3, 50, 2, 'relu')}
ORDER = ('interior', 'before_last', 'last')   # cap - 2 first: the pair that fills the ring to its last row is also what sets `full` (nc == cap under adv = 2)
ACTING_STATES = [pytest.param(True, cap, seq0, id=f'cap{cap}-seq{"0" if not seq0 else "wrap"}') for cap in (7, 8, 9) for seq0 in (0, SEQ_MOD - 6)] + \
                [pytest.param(False, 7, SEQ_MOD - 6, id='not_absorbing-cap7-seqwrap')]


def _ring_end_script(cap, S, absorbing, order=ORDER, seed=SEEDS['acting'], length=None):
  """(next_obs, reward, true_terminal, timeout) per step: true terminations whose transition is stored in the interior slot 2, in slot cap - 1 (absorbing: the
  absorbing -> absorbing row straddles the ring end and lands in slot 0) and in slot cap - 2 (absorbing: the pair fills the ring to its last row, cursor + 2 == cap), in the
  order given; then a step, a timeout and three steps (or as many as `length` asks for). Also the first observation, the reset observations and the slots."""
  slot_of = dict(interior=2, last=cap - 1, before_last=cap - 2)
  flags, cursor = [], 0
  for what in order:
    while cursor % cap != slot_of[what]:
      flags.append((False, False)); cursor += 1
    flags.append((True, False)); cursor += 2 if absorbing else 1
  flags += [(False, False), (False, True)] + [(False, False)] * 3
  while length is not None and len(flags) < length: flags.append((False, False))
  rs = np.random.RandomState(seed)
  script = []
  for term, tout in flags:
    obs = rs.standard_normal(S).astype(np.float32)
    if absorbing: obs[-1] = 0.0
    script.append((obs, float(np.float32(rs.standard_normal())), term, tout))
  first = rs.standard_normal(S).astype(np.float32)
  resets = [rs.standard_normal(S).astype(np.float32) * 0.1 for _ in range(len(order) + 1)]
  if absorbing:
    first[-1] = 0.0
    for r in resets: r[-1] = 0.0
  return script, first, resets, [slot_of[w] for w in order]


def _actor(shape, seed=3):
  S, A, H, depth, activation = shape
  torch.manual_seed(seed)
  actor = P.il.SoftActor(S, A, P.Cfg(hidden_size=H, depth=depth, activation=activation), device=P.DEV)
  actor.flat.copy_(torch.randn_like(actor.flat) * 0.08)
  return actor


def _packed_oracle(ring, S, A):
  """The oracle's struct of arrays as the packed rows of replay.hip (memory.row_layout; the padding floats are zero)."""
  out = np.zeros((ring.size, int(P._lib.lib().il_ring_row_floats(S, A))), np.float32)
  for k, (o, n) in P.il_memory.row_layout(S, A).items():
    out[:, o:o + n] = getattr(ring, k).reshape(ring.size, n)
  return out


def _oracle_ring(cap, S, A, absorbing, script, first, resets, actions, slots, rewards=None):
  """oracle/replay.py through the script with the actions the per-function path took; the cursor in front of every true termination is asserted to be the slot the
  script is built for."""
  ring, obs, k, met = oreplay.ReplayOracle(cap, S, A, absorbing), first, 0, []
  ring.snaps = []   # the packed ring behind every step
  for t, (nxt, rew, term, tout) in enumerate(script, 1):
    if term and not tout: met.append(ring.idx)
    ring.append(t, obs, actions[t - 1], rew if rewards is None else rewards[t - 1], nxt, term, tout)
    if term or tout:
      if absorbing and term and not tout: ring.wrap_for_absorbing_states()
      obs = resets[k]; k += 1
    else: obs = nxt
    ring.snaps.append(_packed_oracle(ring, S, A))
  _met(met == slots, f'the true terminations are meant to be stored in the slots {slots}, not {met}')
  _met(ring.full, 'the script is meant to wrap the ring')
  return ring


def _assert_ring_is_the_oracles(mem, ring, skip=()):
  for k in oreplay.FIELDS:
    if k not in skip: _same_bits(P.N(getattr(mem, k)), getattr(ring, k), f'oracle ring: {k}')
  assert (mem.idx, mem.full, mem.num_trajectories) == (ring.idx, ring.full, ring.num_trajectories)
  assert P.N(mem._ring_state).tolist() == [ring.idx, int(ring.full), ring.size]


_PER_FUNCTION = {}   # the per-function side and the oracle ring, once per (device, shape, ring, absorbing): every schedule and both sequence starts compare with the same arrays


def _per_function_side(name, cap, absorbing):
  key = (str(P.DEV), name, cap, absorbing)
  if key in _PER_FUNCTION: return _PER_FUNCTION[key]
  S, A = ACT_SHAPES[name][:2]
  script, first, resets, slots = _ring_end_script(cap, S, absorbing)
  actor, mem = _actor(ACT_SHAPES[name]), P.il.ReplayMemory(cap, S, A, absorbing, device=P.DEV)
  acts, rings, obs, k = [], [], torch.from_numpy(first).unsqueeze(0), 0
  for t, (nxt, rew, term, tout) in enumerate(script, 1):   # the reference order with the per-function entry points (test_acting_worker_matches_separate_calls)
    a = actor(obs).sample()
    acts.append(P.N(a))
    nxt_t = torch.from_numpy(nxt).unsqueeze(0)
    mem.append(t, obs, a.cpu(), rew, nxt_t, term, tout)
    if term or tout:
      if absorbing and term and not tout: mem.wrap_for_absorbing_states()
      obs = torch.from_numpy(resets[k]).unsqueeze(0); k += 1
    else: obs = nxt_t
    torch.cuda.synchronize()
    rings.append(P.N(mem.ring))   # the ring behind EVERY step: a later append may overwrite what an earlier one got wrong
  actions = np.concatenate(acts)
  oracle = _oracle_ring(cap, S, A, absorbing, script, first, resets, actions, slots)
  _assert_ring_is_the_oracles(mem, oracle)
  for t, (got, want) in enumerate(zip(rings, oracle.snaps), 1): _same_bits(got, want, f'the per-function ring against the oracle behind step {t}')
  out = _PER_FUNCTION[key] = dict(actions=actions, rings=rings, ring=P.N(mem.ring), host=(mem.idx, mem.full, mem.num_trajectories), ring_state=P.N(mem._ring_state), oracle=oracle)
  return out


def _drive(w, schedule, script, first, resets, after_append=None):
  """One ActingWorker through the script in one of its three schedules; returns the actions. Overlap: every append launch is enqueued a second time without a new post on
  the step whose post wrapped the sequence and on every true termination (the straddling one among them): the replay must append nothing. `after_append(t)`: called
  behind every append."""
  acts, k, mem = [], 0, w.memory
  replayed_on_the_wrap = False

  def appended(t, box):
    torch.cuda.synchronize()   # the device's cursor and `full` behind EVERY append, against the host's arithmetic mirror: `full` is sticky, the end of the run cannot show when it was set
    assert P.N(mem._ring_state).tolist() == [mem.idx, int(mem.full), mem.size], f'step {t}: the device ring state'
    if after_append: after_append(t, box)
  if schedule == 'exact':
    obs = first
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts.append(P.N(w.act(obs)))
      w.append(t, nxt, rew, term, tout)
      appended(t, w._append_box)
      if term or tout: obs = resets[k]; k += 1
      else: obs = nxt
  elif schedule == 'fused':
    a = w.act(first)
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts.append(P.N(a))
      ended = term or tout
      a = w.step(t, nxt, rew, term, tout, obs=resets[k] if ended else None)
      appended(t, w._act_box)
      k += int(ended)
  else:
    obs, a, last_post = first, w.act(first), w._seq
    for t, (nxt, rew, term, tout) in enumerate(script, 1):
      acts.append(P.N(a))
      w.post(t, obs, a, nxt, rew, term, tout)
      wrapped, last_post = w._seq < last_post, w._seq
      w.enqueue_append()
      appended(t, w._append_box)
      if wrapped or term:
        torch.cuda.synchronize()
        before = P.N(mem.ring), P.N(mem._ring_state)
        w.enqueue_append()   # a replayed launch without a new post
        torch.cuda.synchronize()
        _same_bits(P.N(mem.ring), before[0], f'step {t}: a replayed append changed the ring')
        np.testing.assert_array_equal(P.N(mem._ring_state), before[1], err_msg=f'step {t}: a replayed append moved the cursor')
        replayed_on_the_wrap |= wrapped
      ended = term or tout
      obs = resets[k] if ended else nxt
      k += int(ended)
      a = w.act(obs)
    w.replayed_on_the_wrap = replayed_on_the_wrap
  torch.cuda.synchronize()
  return np.concatenate(acts)


ACTING_WORKERS = [pytest.param(schedule, name, id=f'{schedule}-{name}') for name in ACT_SHAPES for schedule in ('exact', 'fused', 'overlap') if (schedule, name) != ('overlap', 'general_layers')]


@pytest.mark.parametrize('absorbing,cap,seq0', ACTING_STATES)
@pytest.mark.parametrize('schedule,name', ACTING_WORKERS)
def test_acting_worker_at_the_ring_end_and_the_sequence_wrap(schedule, name, absorbing, cap, seq0):
  """il.ActingWorker in its three schedules (il_act_step; il_act_step_general in both forms - the layer-at-a-time form has no overlap schedule) into rings of 7, 8 and 9 rows,
  with true terminations stored in slot 2, in slot cap - 1 (act_append's `(p.cursor + 1) % p.cap` wraps: act_mail.hpp:76) and in slot cap - 2 (act_commit's nc == cap under
  adv = 2: act_mail.hpp:88-90), the commit sequence started at 0 and six posts below its wrap (acting.py:188): the actions, the whole ring, cursor / full / trajectory count
  and the device's ring state are the per-function path's, and that path's ring is oracle/replay.py's. One case without absorbing states ends an episode in slot cap - 1."""
  assert P.il.acting._SEQ_MOD == SEQ_MOD
  side = _per_function_side(name, cap, absorbing)
  S, A = ACT_SHAPES[name][:2]
  script, first, resets, _ = _ring_end_script(cap, S, absorbing)
  actor, mem = _actor(ACT_SHAPES[name]), P.il.ReplayMemory(cap, S, A, absorbing, device=P.DEV)
  w = P.il.ActingWorker(actor, mem, mirror=schedule == 'overlap')
  assert w.general == (name != 'fused') and w.one_launch == (name != 'general_layers')
  w._seq = seq0
  actions = _drive(w, schedule, script, first, resets, after_append=lambda t, box: _same_bits(P.N(mem.ring), side['rings'][t - 1], f'the ring behind step {t}'))
  np.testing.assert_array_equal(side['actions'], actions)
  _same_bits(P.N(mem.ring), side['ring'], 'the ring')
  assert side['host'] == (mem.idx, mem.full, mem.num_trajectories)
  np.testing.assert_array_equal(P.N(mem._ring_state), side['ring_state'])
  _assert_ring_is_the_oracles(mem, side['oracle'])
  if seq0:
    assert 0 < w._seq < seq0, 'the sequence is meant to wrap'
    if schedule == 'overlap': _met(w.replayed_on_the_wrap, 'a replayed append is meant to fall on the post that wrapped the sequence')
  else: assert w._seq > 0


test_acting_worker_at_the_ring_end_and_the_sequence_wrap.streams = True

POP_ORDERS = (('last',), ('before_last',), ('interior',))   # learner 0 straddles the ring end, learner 1 fills the ring to its last row, learner 2 does neither
PWIL_CFG = dict(state_only=False, reward_scale=5, reward_bandwidth_scale=5)
PWIL_ATOMS = (600, 40)                   # the smallest atom set of tests/test_pwil_acting_gpu.py: 600 atoms, horizon 40
PWIL_SHAPE = (12, 3, 64, 2, 'relu')      # its shipped actor shape at Hopper dims


def _pwil_discriminator(seed, shape=PWIL_SHAPE):
  S, A = shape[:2]
  n, horizon = PWIL_ATOMS
  atoms, _ = gi.pwil_case(seed, n, S + A, 1)
  expert = P.il.ReplayMemory(n, S, A, False, transitions=dict(states=torch.from_numpy(atoms[:, :S]), actions=torch.from_numpy(atoms[:, S:]), rewards=torch.zeros(n),
                                                              next_states=torch.from_numpy(atoms[:, :S]), terminals=torch.zeros(n), timeouts=torch.zeros(n), weights=torch.ones(n),
                                                              num_trajectories=4), device=P.DEV)
  return P.il.PWILDiscriminator(S, A, P.Cfg(**PWIL_CFG), expert, horizon)


def _coupled_word(carry, S, A):
  """act_carry_coupled (act_mail.hpp:28): the commit word of the post il_pwil_act_reward computed the reward for, as raw bits."""
  return int(P.N(carry)[S + A + 2:S + A + 3].view(np.uint32)[0])


def _population_body(schedule, cap, seq0, shape, pwil):
  S, A, L = shape[0], shape[1], 3
  scripts = [_ring_end_script(cap, S, True, order=POP_ORDERS[l], seed=100 + l, length=2 * cap + 4) for l in range(L)]
  steps = 2 * cap + 4
  assert all(len(s[0]) == steps for s in scripts)
  seeds = [1000 + 17 * l for l in range(L)]
  actors_a, actors_b = [_actor(shape, 11 + l) for l in range(L)], [_actor(shape, 11 + l) for l in range(L)]
  mems_a, mems_b = ([P.il.ReplayMemory(cap, S, A, True, device=P.DEV) for _ in range(L)] for _ in range(2))
  discs_a, discs_b = ([_pwil_discriminator(41 + l, shape) for l in range(L)] if pwil else None for _ in range(2))
  rs = np.random.RandomState(77)
  eval_obs = [[rs.standard_normal(S).astype(np.float32) for _ in range(L)] for _ in range(steps)]

  want_acts, want_eval, want_rings = [], [], []
  for l in range(L):   # the reference: learner l alone, its sequence from 0
    greedy, rings = [], []

    def evaluate(t, box, l=l, greedy=greedy, rings=rings):
      rings.append(P.N(mems_a[l].ring))   # (behind _drive's synchronisation) the ring behind EVERY step
      if t % 3 == 0: greedy.append(P.N(actors_a[l].get_greedy_action(torch.from_numpy(eval_obs[t - 1][l]))))
    single = P.il.ActingWorker(actors_a[l], mems_a[l], noise_seed=seeds[l], reward_model=discs_a[l] if pwil else None)
    want_acts.append(_drive(single, schedule, *scripts[l][:3], after_append=evaluate))
    want_eval.append(greedy); want_rings.append(rings)
    oracle = _oracle_ring(cap, S, A, True, *scripts[l][:3], want_acts[l], scripts[l][3])
    _assert_ring_is_the_oracles(mems_a[l], oracle, skip=('rewards',) if pwil else ())
    o_rew = 2 * S + A
    for t, (got, want) in enumerate(zip(rings, oracle.snaps), 1):   # the reward column of a PWIL learner is its coupling's: compared with the worker's, not with the script's
      _same_bits(np.delete(got, o_rew, axis=1) if pwil else got, np.delete(want, o_rew, axis=1) if pwil else want, f'learner {l} alone against the oracle behind step {t}')

  w = P.il.PopulationActingWorker(actors_b, mems_b, seeds, reward_models=discs_b)
  w._seq = w._eval_seq = seq0
  acts, evals, k, words = [[] for _ in range(L)], [[] for _ in range(L)], [0] * L, []
  obs = [s[1] for s in scripts]
  pending = w.act(obs) if schedule == 'fused' else None
  for t in range(1, steps + 1):
    tr = [scripts[l][0][t - 1] for l in range(L)]
    follow = []
    for l, (nxt, rew, term, tout) in enumerate(tr):
      if term or tout:
        follow.append(scripts[l][2][k[l]]); k[l] += 1
      else: follow.append(nxt)
    columns = [[x[i] for x in tr] for i in range(4)]
    if schedule == 'exact':
      a = w.act(obs)
      w.append(t, *columns)
      box = w._append_box
    else:
      a = pending
      pending = w.step(t, *columns, obs=follow)
      box = w._act_box
    torch.cuda.synchronize()
    for l, m in enumerate(mems_b):
      assert P.N(m._ring_state).tolist() == [m.idx, int(m.full), m.size], f'step {t}, learner {l}: the device ring state'
      _same_bits(P.N(m.ring), want_rings[l][t - 1], f'step {t}: the ring of learner {l}')
    if pwil:
      for l in range(L): assert _coupled_word(w.carry[l], S, A) == int(box.words[l]), f'step {t}, learner {l}: the coupled word'
      words.append(int(box.words[0]))
    for l in range(L): acts[l].append(P.N(a[l:l + 1]))
    if t % 3 == 0:
      g = w.act_eval(eval_obs[t - 1])
      for l in range(L): evals[l].append(P.N(g[l:l + 1]))
    obs = follow
  torch.cuda.synchronize()
  for l in range(L):
    np.testing.assert_array_equal(want_acts[l], np.concatenate(acts[l]), err_msg=f'actions of learner {l}')
    np.testing.assert_array_equal(np.concatenate(want_eval[l]), np.concatenate(evals[l]), err_msg=f'evaluation actions of learner {l}')
    _same_bits(P.N(mems_b[l].ring), P.N(mems_a[l].ring), f'ring of learner {l}')
    np.testing.assert_array_equal(P.N(mems_a[l]._ring_state), P.N(mems_b[l]._ring_state), err_msg=f'device cursor of learner {l}')
    assert (mems_a[l].idx, mems_a[l].full, mems_a[l].num_trajectories) == (mems_b[l].idx, mems_b[l].full, mems_b[l].num_trajectories), l
    assert actors_a[l]._act_calls == actors_b[l]._act_calls, l
    if pwil: _same_bits(P.N(discs_b[l].expert_weights), P.N(discs_a[l].expert_weights), f'atom weights of learner {l}')
  _met(not np.array_equal(P.N(mems_b[0].ring), P.N(mems_b[1].ring)), 'the learners are meant to differ')
  if seq0:
    assert 0 < w._seq < seq0 and 0 < w._eval_seq < seq0, 'both sequences are meant to wrap'
    if pwil: _met(any(b < a for a, b in zip(words, words[1:])), 'the coupled word is meant to be compared across the wrap')


@pytest.mark.parametrize('seq0', [0, SEQ_MOD - 6], ids=['seq0', 'seqwrap'])
@pytest.mark.parametrize('cap', [7, 8, 9])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_population_acting_at_the_ring_end_and_the_sequence_wrap(schedule, cap, seq0):
  """il.PopulationActingWorker (il_act_step_population), three learners in lockstep whose first true terminations are stored in slot cap - 1, slot cap - 2 and slot 2, `_seq`
  AND `_eval_seq` started six posts below the wrap (acting.py:405, 409) and a greedy evaluation act of all learners between two appends, every third step: each learner's
  actions, ring, cursor and Philox counter are those of its own ActingWorker (sequence from 0, `get_greedy_action` where the population evaluates), and that worker's ring
  is oracle/replay.py's."""
  _population_body(schedule, cap, seq0, ACT_SHAPES['fused'], pwil=False)


test_population_acting_at_the_ring_end_and_the_sequence_wrap.streams = True

_PWIL_SIDE = {}


def _pwil_per_function_side(cap):
  """train.py's per-function PWIL loop (tests/test_pwil_acting_gpu.py _per_function_side) over the ring-end script, once per ring size."""
  key = (str(P.DEV), cap)
  if key in _PWIL_SIDE: return _PWIL_SIDE[key]
  S, A = PWIL_SHAPE[:2]
  script, first, resets, slots = _ring_end_script(cap, S, True)
  actor, disc, mem = _actor(PWIL_SHAPE), _pwil_discriminator(41), P.il.ReplayMemory(cap, S, A, True, device=P.DEV)
  acts, rewards, rings, obs, k = [], [], [], torch.from_numpy(first).unsqueeze(0), 0
  for t, (nxt, rew, term, tout) in enumerate(script, 1):
    a = actor(obs).sample()
    acts.append(P.N(a))
    reward = disc.compute_reward(obs, a)
    rewards.append(float(reward))
    nxt_t = torch.from_numpy(nxt).unsqueeze(0)
    mem.append(t, obs, a, reward, nxt_t, term, tout)
    if term or tout:
      if term and not tout: mem.wrap_for_absorbing_states()
      disc.reset()
      obs = torch.from_numpy(resets[k]).unsqueeze(0); k += 1
    else: obs = nxt_t
    torch.cuda.synchronize()
    rings.append(P.N(mem.ring))
  actions = np.concatenate(acts)
  oracle = _oracle_ring(cap, S, A, True, script, first, resets, actions, slots, rewards=rewards)
  _assert_ring_is_the_oracles(mem, oracle)
  for t, (got, want) in enumerate(zip(rings, oracle.snaps), 1): _same_bits(got, want, f'the per-function ring against the oracle behind step {t}')
  _met(len(set(rewards)) > len(rewards) // 2 and all(r > 0 for r in rewards), 'the coupling is meant to give every step a reward of its own')
  out = _PWIL_SIDE[key] = dict(actions=actions, rings=rings, ring=P.N(mem.ring), weights=P.N(disc.expert_weights), host=(mem.idx, mem.full, mem.num_trajectories), oracle=oracle)
  return out


@pytest.mark.parametrize('seq0', [0, SEQ_MOD - 6], ids=['seq0', 'seqwrap'])
@pytest.mark.parametrize('cap', [7, 8, 9])
@pytest.mark.parametrize('schedule', ['exact', 'fused', 'overlap'])
def test_pwil_coupling_at_the_ring_end_and_the_sequence_wrap(schedule, cap, seq0):
  """ActingWorker(reward_model=PWILDiscriminator): il_pwil_act_reward in front of every appending launch, 600 atoms, the ring-end script, the sequence from 0 and from six
  posts below its wrap. Behind every append the coupled word in the carry (act_carry_coupled) is the commit word of that post - across the wrap, where it goes from
  131071 * 64 + flags down to 64 + flags; actions, ring (reward column included), atom weights and cursor are the per-function loop's, whose ring is the oracle's."""
  side = _pwil_per_function_side(cap)
  S, A = PWIL_SHAPE[:2]
  script, first, resets, _ = _ring_end_script(cap, S, True)
  actor, disc, mem = _actor(PWIL_SHAPE), _pwil_discriminator(41), P.il.ReplayMemory(cap, S, A, True, device=P.DEV)
  w = P.il.ActingWorker(actor, mem, mirror=schedule == 'overlap', reward_model=disc)
  w._seq = seq0
  words = []

  def coupled(t, box):
    torch.cuda.synchronize()
    assert _coupled_word(w.carry, S, A) == int(box.word), f'step {t}: the coupled word'
    _same_bits(P.N(mem.ring), side['rings'][t - 1], f'the ring behind step {t}')
    words.append(int(box.word))
  actions = _drive(w, schedule, [(nxt, 1e9, term, tout) for nxt, _, term, tout in script], first, resets, after_append=coupled)   # the reward argument is the caller's: it must not reach the ring
  np.testing.assert_array_equal(side['actions'], actions)
  _same_bits(P.N(mem.ring), side['ring'], 'the ring')
  _same_bits(P.N(disc.expert_weights), side['weights'], 'the atom weights')
  assert side['host'] == (mem.idx, mem.full, mem.num_trajectories)
  _assert_ring_is_the_oracles(mem, side['oracle'])
  if seq0:
    assert 0 < w._seq < seq0, 'the sequence is meant to wrap'
    _met(any(b < a for a, b in zip(words, words[1:])), 'the coupled word is meant to be compared across the wrap')
    if schedule == 'overlap': _met(w.replayed_on_the_wrap, 'a replayed pair is meant to fall on the post that wrapped the sequence')


test_pwil_coupling_at_the_ring_end_and_the_sequence_wrap.streams = True


@pytest.mark.parametrize('seq0', [0, SEQ_MOD - 6], ids=['seq0', 'seqwrap'])
@pytest.mark.parametrize('cap', [7, 8, 9])
@pytest.mark.parametrize('schedule', ['exact', 'fused'])
def test_pwil_population_coupling_at_the_ring_end_and_the_sequence_wrap(schedule, cap, seq0):
  """il_pwil_act_reward_population in front of il_act_step_population: the population body above with one PWILDiscriminator (600 atoms of its own) per learner; every
  learner's coupled word is its commit word behind every append, its atom weights and its reward column are those of its own ActingWorker(reward_model=...)."""
  _population_body(schedule, cap, seq0, PWIL_SHAPE, pwil=True)


test_pwil_population_coupling_at_the_ring_end_and_the_sequence_wrap.streams = True


# ================================================================================================ 3. behind the grid caps
WIDE = (40, 17)          # a packed row of 104 floats = 26 lanes of 16 bytes
MIX_N = 5200             # 5200 x 26 = 135,200 lanes > 512 x 256: the grid-stride loops of replay.hip:79, 140 and 163 run a second trip (mix_copy_expert carries its column: `c += dc`)
MIX_FREQ, MIX_STEP = 1250, 4001   # AdRIL: round 4 (ceil(4001 / 1250)); the rows are stamped over rounds 1 .. 4, both sides of every multiple of 1250 among them


def _mix_case(label, seed):
  """(policy rows, expert rows) of MIX_N packed rows at WIDE, step stamps around the round edges; the four n_expert of the issue with their dyn words and reward_expert."""
  S, A = WIDE
  row, o_rew = int(P._lib.lib().il_ring_row_floats(S, A)), 2 * S + A
  assert row == 104 and MIX_N * (row // 4) > 512 * 256
  rs = np.random.RandomState(seed)
  pol, exp = rs.standard_normal((MIX_N, row)).astype(np.float32), (rs.standard_normal((MIX_N, row)) + 3).astype(np.float32)
  edge = np.array([1, 1249, 1250, 1251, 2499, 2500, 2501, 3749, 3750, 3751, 4000, 4001], np.float32)
  pol[:, o_rew + 4] = np.where(rs.uniform(size=MIX_N) < 0.5, edge[rs.randint(0, len(edge), MIX_N)], rs.randint(1, 4002, MIX_N).astype(np.float32))
  exp[:, o_rew + 4] = rs.randint(1, 5000, MIX_N).astype(np.float32)
  round_num = -(-MIX_STEP // MIX_FREQ) if label == 2 else 0
  learners = [(ne, [ne, round_num, traj], float(np.float32(1 / (3 + l)))) for l, (ne, traj) in enumerate(((MIX_N // 2, 7), (MIX_N, 0), (0, 1000003), (MIX_N - 100, 12)))]
  return pol, exp, learners, row, o_rew


def _numpy_mix_relabel(pol, exp, n_expert, label, traj, expert_traj_reward, o_rew):
  """models.py:287-318 on packed rows, for any n_expert: the lines of oracle/adril.py (mix; RelabellerOracle.resample_and_relabel from `r = transitions['rewards']` on)."""
  f32 = np.float32
  out = pol.copy()
  out[:n_expert] = exp[:n_expert]
  r = out[:, o_rew]
  if label == 2:
    r[:n_expert] = f32(expert_traj_reward)
    round_num = -(-MIX_STEP // MIX_FREQ)
    row_round = np.ceil(out[n_expert:, o_rew + 4].astype(f32) / f32(MIX_FREQ))
    r[n_expert:] = (f32(-1) * (f32(round_num) > row_round).astype(f32)) / f32(max(traj, 1))
  elif label == 1:
    r[:n_expert] = 1
    r[n_expert:] = 0
  return out


def _guarded(values, offset=0):
  """[n, row] values between guard floats, `offset` floats off the 16-byte grid: (buffer, view of the rows inside it)."""
  n, row = values.shape
  buf = torch.full((GUARD + offset + n * row + GUARD,), SENTINEL, dtype=torch.float32).to(P.DEV)
  rows = buf[GUARD + offset:GUARD + offset + n * row].view(n, row)
  rows.copy_(P.T(values))
  assert rows.data_ptr() % 16 == 4 * offset
  return buf, rows


def _assert_guards(buf, n_floats, what, offset=0):
  b = P.N(buf)
  assert (b[:GUARD + offset] == SENTINEL).all() and (b[GUARD + offset + n_floats:] == SENTINEL).all(), f'{what}: a guard float was written'


@pytest.mark.parametrize('label', [0, 1, 2], ids=['label0-mix', 'label1-SQIL', 'label2-AdRIL'])
def test_mix_relabel_launches_behind_the_grid_cap(label):
  """il_batch_mix_relabel_population (four learners in one launch: n_expert = n / 2, n, 0 and n - 100), il_batch_mix_relabel_dyn and il_batch_mix_relabel per learner, at
  5200 rows of 26 lanes - 135,200 lanes, behind the cap of 512 workgroups: every float of every learner's rows through an int32 view against the numpy statement of
  models.py:287-318 and against each other, the guard floats on both sides untouched, the expert rows unchanged; the halves, the expert turn and the policy turn also
  against oracle/adril.py's RelabellerOracle itself."""
  S, A = WIDE
  pol, exp, learners, row, o_rew = _mix_case(label, SEEDS['mix'] + label)
  freq = MIX_FREQ if label == 2 else 0
  want = [_numpy_mix_relabel(pol, exp, ne, label, dyn[2], re, o_rew) for ne, dyn, re in learners]
  if label:   # the oracle class itself where it has the case: unbalanced halves, a balanced expert turn, a balanced policy turn
    views = lambda rows: dict(rewards=rows[:, o_rew], step=rows[:, o_rew + 4], rest=rows)
    for l, (balanced, sample_expert) in enumerate(((False, True), (True, True), (True, False))):
      orel = oadril.RelabellerOracle(freq, balanced); orel.sample_expert = sample_expert
      p, e = pol.copy(), exp.copy()
      tr = views(p)
      n_expert = orel.resample_and_relabel(tr, views(e), MIX_STEP, learners[l][1][2], round(1 / learners[l][2]))
      assert n_expert == learners[l][0]
      got = tr['rest'].copy(); got[:, o_rew] = tr['rewards']; got[:, o_rew + 4] = tr['step']
      _same_bits(got, want[l], f'the numpy statement against RelabellerOracle, learner {l}')
  if label == 2:
    r = want[2][:, o_rew]
    _met((_bits(r) == -2 ** 31).sum() > 100 and (r < 0).sum() > 100, 'rows of the current round (-0.0) and older rows are both meant to occur')
  p, L_ = P._lib.ptr, P._lib.lib()
  erows = P.T(exp)
  # one launch for the four learners
  dev = [_guarded(pol) for _ in learners]
  dyn = torch.tensor([d for _, d, _ in learners], dtype=torch.int64).to(P.DEV)
  descs = P.il_training._device_array([P._lib.MixLearner(rows.data_ptr(), erows.data_ptr(), dyn[l].data_ptr(), re) for l, ((_, rows), (_, _, re)) in enumerate(zip(dev, learners))], P.DEV)
  P._lib.check(L_.il_batch_mix_relabel_population(p(descs), len(learners), MIX_N, S, A, label, freq, P._lib.stream_ptr()))
  torch.cuda.synchronize()
  for l, (buf, rows) in enumerate(dev):
    _same_bits(P.N(rows), want[l], f'population launch, learner {l} (n_expert {learners[l][0]})')
    _assert_guards(buf, MIX_N * row, f'population launch, learner {l}')
  for l, (ne, d, re) in enumerate(learners):   # the one-learner launches: words from device memory, and as arguments
    buf, rows = _guarded(pol)
    P._lib.check(L_.il_batch_mix_relabel_dyn(p(rows), p(erows), MIX_N, S, A, label, freq, re, p(dyn[l]), P._lib.stream_ptr()))
    torch.cuda.synchronize()
    _same_bits(P.N(rows), want[l], f'il_batch_mix_relabel_dyn, n_expert {ne}'); _assert_guards(buf, MIX_N * row, f'il_batch_mix_relabel_dyn, n_expert {ne}')
    buf, rows = _guarded(pol)
    P._lib.check(L_.il_batch_mix_relabel(p(rows), p(erows), MIX_N, S, A, ne, label, freq, d[1], re, d[2], P._lib.stream_ptr()))
    torch.cuda.synchronize()
    _same_bits(P.N(rows), want[l], f'il_batch_mix_relabel, n_expert {ne}'); _assert_guards(buf, MIX_N * row, f'il_batch_mix_relabel, n_expert {ne}')
  _same_bits(P.N(erows), exp, 'the expert rows')


def test_mix_relabel_population_behind_the_grid_cap_off_the_16_byte_grid():
  """The same launch with row buffers one float off the 16-byte grid: the one-float lanes of mix_copy_expert, 5200 x 104 = 540,800 of them, four trips behind the cap."""
  S, A = WIDE
  pol, exp, learners, row, o_rew = _mix_case(2, SEEDS['mix'] + 7)
  learners = [learners[0], learners[3]]
  want = [_numpy_mix_relabel(pol, exp, ne, 2, dyn[2], re, o_rew) for ne, dyn, re in learners]
  dev = [_guarded(pol, offset=1) for _ in learners]
  ebuf, erows = _guarded(exp, offset=1)
  dyn = torch.tensor([d for _, d, _ in learners], dtype=torch.int64).to(P.DEV)
  descs = P.il_training._device_array([P._lib.MixLearner(rows.data_ptr(), erows.data_ptr(), dyn[l].data_ptr(), re) for l, ((_, rows), (_, _, re)) in enumerate(zip(dev, learners))], P.DEV)
  P._lib.check(P._lib.lib().il_batch_mix_relabel_population(P._lib.ptr(descs), 2, MIX_N, S, A, 2, MIX_FREQ, P._lib.stream_ptr()))
  torch.cuda.synchronize()
  for l, (buf, rows) in enumerate(dev):
    _same_bits(P.N(rows), want[l], f'learner {l}'); _assert_guards(buf, MIX_N * row, f'learner {l}', offset=1)
  _same_bits(P.N(erows), exp, 'the expert rows')


ROWS_CAP, ROWS_N = 4000, 3500   # 3500 x 104 = 364,000 floats > 1024 x 256: k_write_rows behind its cap, across the ring end (cursor cap - 10)


def _wide_transitions(seed, n):
  S, A = WIDE
  return gi.transitions(np.random.RandomState(seed), n, S, A, terminal_frac=0.05, weighted=True)


def _torch_transitions(tr, traj):
  return {**{k: torch.from_numpy(v) for k, v in tr.items() if k != 'absorbing'}, 'num_trajectories': traj}


_WRITE_ROWS = {}


def _write_rows_reference():
  """oracle/replay.py: a ring of 4000 rows holding 3990, then 3500 sequential appends (transfer_transitions). Once for both tests."""
  if not _WRITE_ROWS:
    S, A = WIDE
    pre, src = _wide_transitions(SEEDS['rows'], ROWS_CAP - 10), _wide_transitions(SEEDS['rows'] + 1, ROWS_N)
    odst = oreplay.ReplayOracle(ROWS_CAP, S, A, True, transitions={**pre, 'num_trajectories': 2})
    osrc = oreplay.ReplayOracle(ROWS_N, S, A, True, transitions={**src, 'num_trajectories': 3})
    _met(odst.idx == ROWS_CAP - 10 and not odst.full, 'the cursor is meant to stand ten rows in front of the ring end')
    odst.transfer_transitions(osrc)
    _met(odst.full and odst.idx == ROWS_N - 10, 'the appends are meant to cross the ring end')
    _WRITE_ROWS.update(pre=pre, src=src, oracle=odst)
  return _WRITE_ROWS['pre'], _WRITE_ROWS['src'], _WRITE_ROWS['oracle']


@pytest.mark.parametrize('how', ['il_replay_write_rows', 'transfer_transitions'])
def test_write_rows_behind_the_grid_cap_across_the_ring_end(how):
  """3500 rows of 104 floats at cursor cap - 10 of a ring of 4000: k_write_rows' `(cursor + r) % capacity` (replay.hip:39) behind the cap of 1024 workgroups, against 3500
  sequential appends of oracle/replay.py - through the entry point, and through ReplayMemory.transfer_transitions with its host-side cursor."""
  S, A = WIDE
  pre, src, oracle = _write_rows_reference()
  dst = P.il.ReplayMemory(ROWS_CAP, S, A, True, transitions=_torch_transitions(pre, 2), device=P.DEV)
  smem = P.il.ReplayMemory(ROWS_N, S, A, True, transitions=_torch_transitions(src, 3), device=P.DEV)
  assert dst.row == 104 and ROWS_N * dst.row > 1024 * 256 and (dst.idx, dst.full) == (ROWS_CAP - 10, False)
  if how == 'transfer_transitions':
    dst.transfer_transitions(smem)
    assert (dst.idx, dst.full, dst.num_trajectories) == (oracle.idx, oracle.full, oracle.num_trajectories)
    assert P.N(dst._ring_state).tolist() == [oracle.idx, 1, ROWS_CAP]
  else:
    rows = smem.ring.clone()
    rows[:, dst.layout['weights'][0]] = 1.0   # memory.py:46-48 re-appends without the weights
    P._lib.check(P._lib.lib().il_replay_write_rows(P._lib.ptr(dst.ring), ROWS_CAP, dst.row, ROWS_CAP - 10, P._lib.ptr(rows), ROWS_N, P._lib.stream_ptr()))
  torch.cuda.synchronize()
  for k in oreplay.FIELDS:
    _same_bits(P.N(getattr(dst, k)), getattr(oracle, k), k)


def test_gather_behind_the_grid_cap():
  """il_replay_gather of 12000 rows of 26 lanes (312,000 lanes > 1024 x 256) from a ring of 4000, the indices 0 and cap - 1 among them at both ends of the batch and in
  the second trip: fancy indexing, guard floats behind the rows."""
  S, A = WIDE
  n, cap = 12000, ROWS_CAP
  mem = _filled_ring(cap, S, A, 0, True, SEEDS['rows'] + 2)
  assert n * (mem.row // 4) > 1024 * 256
  idx = np.random.RandomState(SEEDS['rows'] + 3).randint(0, cap, n).astype(np.int32)
  idx[[0, 1, n // 2, 10100, n - 2, n - 1]] = [cap - 1, 0, cap - 1, 0, 0, cap - 1]
  out = torch.full((n * mem.row + GUARD,), SENTINEL, dtype=torch.float32).to(P.DEV)
  P._lib.check(P._lib.lib().il_replay_gather(P._lib.ptr(mem.ring), cap, mem.row, P._lib.ptr(P.T(idx)), n, P._lib.ptr(out), P._lib.stream_ptr()))
  torch.cuda.synchronize()
  got = P.N(out)
  _same_bits(got[:n * mem.row].reshape(n, mem.row), P.N(mem.ring)[idx], 'gathered rows')
  assert (got[n * mem.row:] == SENTINEL).all()
  _same_bits(P.N(mem.gather(torch.from_numpy(idx))), P.N(mem.ring)[idx], 'ReplayMemory.gather')


# ================================================================================================ 4. k_g_pack_sac behind its cap
def test_general_sac_update_behind_the_pack_cap():
  """il_sac_update_general, layer at a time (hidden 17, depth 2, tanh: no ReLU, no kink), two updates at (S, A) = (111, 8), B = 576: of k_g_pack_sac's five input matrices the critic's
  (s, a) matrix (blockIdx.y == 3, general.hip:180) holds (S + A) x B = 68,544 floats and takes a second grid-stride trip behind the cap of 256 workgroups (general.hip:1009); the
  four state matrices hold S x B = 63,936 and stay in front of it. The body and the bounds of tests/test_size_edges_gpu.py::test_general_sac_update_at_edge_sizes."""
  dims, B = (111, 8), 576
  assert (dims[0] + dims[1]) * B > 256 * 256
  c = gi.sac_case(seed=SEEDS['sac'], env=dims, hidden=17, batch=B, steps=2, depth=2, activation='tanh')
  with _recording():
    actor, critic = Z._sac_updates('general SAC', c, dims)
  assert actor.general and critic.general
