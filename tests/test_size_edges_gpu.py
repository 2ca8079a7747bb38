"""`-m gpu`: every kernel family against its oracle at the batch sizes and hidden widths the rest of the suite never runs (tests/golden/inputs.py EDGE_BATCHES and
EDGE_HIDDEN_*): batches of 1, 2 and 3 rows, every B mod 4, both sides of 16 / 32 / 64 / 128, and hidden widths at the limits of each entry point and off its 16- and
64-wide tiles. One or two steps at the narrow widths (11, 3) / (17, 6) (`imitation.absorbing=false`: odd, fields off the 16-byte grid) and one case per family at
(1, 1). Each body is its sibling in tests/test_gpu_parity.py / tests/test_dim_edges_gpu.py with `batch` and `hidden` free and the sibling's bounds, unchanged;
tests/test_size_edges_emulated.py runs the same bodies on the host emulation of the kernels. Batches and widths are paired (`_pairs`), not crossed: every batch and every
width of a family occurs at least twice. Everything device-side is reached through the names of tests/test_gpu_parity.py (`P.il`, `P.T`, `P.close`, ...), which the
emulated run rebinds to the CPU.

Also here: `il.sac_update` / `behavioural_cloning_update` / `PretrainPlan('BC')` with the fused network shape at a batch that is not a multiple of 16 (train.py's
per-function path: routed through csrc/general.hip), and one refusal per limit of a hidden width - loud or correct, never silent.

What an odd B or H changes that the emulator cannot see is alignment. Every 16-byte (`f32x4`) access of these kernels whose address depends on B or H, and what keeps it
aligned (read before the first run on the card; no site was found without a guard):
  general.hip  k_g_linear / k_g_bwd / k_g_dw / k_gt_fwd / k_gt_bwd stores and loads `XT + net * ns + k * Bp + row0 + 4 * g`: Bp = g_bp(B) rounds B up to 16, row0 is a
               multiple of 16, every net stride is a multiple of Bp, every slab of the workspace starts at g_sac_ws / g_act_ws `take` (offsets rounded up to 4 floats);
  general.hip  k_gt_dw / k_gt_dw32 batch lanes `zr + r0 (+ 16 u)`: the same [feature][Bp] slabs; the 32 x 32 block jobs only when Bp % 128 == 0 (DWS_ROWS);
  general.hip  target step in the optimiser tail: `(polyak_n & 3) == 0 && (target & 15) == 0 && (polyak_src & 15) == 0`, else the scalar loop;
  general.hip  k_gt_repack `W2 + (n + r) * H + k` and the lane-ordered copies: gt_packable - H % 64 == 0, layer offsets `(L.oW & 3) == 0`, arena `& 15` (and `(Ps & 3) == 0`);
  general.hip / mlp_tile.hpp  LDS operands `Xs + j * ldx + 4 * g + k0`: ldx = round_up16(K) + 4 or H + 4 with H % 16 == 0 (gt_shape_ok), LDS regions in multiples of 4 floats;
  mlp_tile.hpp tile_fwd weight lanes: `aligned = (ldw & 3) == 0 && (W & 15) == 0` picks load4<0 / 1>, anything else the four clamped dword loads of load4<2>;
               l1_prefetch only under l1_rows_aligned (`(Kw & 3) == 0 && (W & 15) == 0`), w1_issue reads whole lanes of a 16-byte aligned W (H * S + H a multiple of 4: H % 64 == 0);
  mlp_tile.hpp tile_packed / tile_pair `pp + (kb + u) * 256`: the copies k_gt_repack / k_repack wrote, 256-float blocks in a slab at a `take` offset;
  dw_block.hpp dw32 `dzT + f * B + rr`, `gload4(params + eo)`: B % 128 == 0 there, rr a multiple of 4, and `full || flat || rowg` (whole, 16-byte aligned rows) before a vector access of p / m / v;
  disc_reward.hpp dot4 / dot_strided / disc_pload4: LDS rows of Dp + 4 floats (Dp = roundup4(D)), H % 16 == 0 (il_disc refuses every other width: test below), flat lanes
               of W1 only under disc_w1_flat_ok (`(W1 & 15) == 0 && ((H * D) & 3) == 0`);
  gail_deep_tile.hpp, gail_deep.hip, gail_shaped.hip, gail_shaped_deep.hip, red.hip, dril.hip: no 16-byte access at all (dword loads and stores only).

Seeds (tests/test_dim_edges_gpu.py SEEDS): ONE base per family, fixed, for which every case below stays inside its bounds on the emulated kernels; every case runs at
base + its sizes, nothing is drawn again or filtered. Bases that were tried and rejected, and why:
  shaped_deep - none rejected. The seed the issue reports, `gail_shaped_deep` at (B 65, H 128, depth 1, relu), seed 1030 + 65, fails only at (11, 3) with the builder's
    absorbing column left in place: 11 gradient elements, flat index 24 and 242 .. 251 (62 x the bound on the emulated kernels), all of hidden unit 9 of the potential
    (h.0.bias[9], h.0.weight[9, 0:10]), whose pre-activation is 2.4e-8 of the layer's scale at one row of the oracle's own forward - a ReLU that two correct float32
    evaluations put on different sides. `_kink_units` is that check, test_the_rejected_shaped_deep_seed_is_a_relu_kink asserts it. The cell runs here like its siblings,
    with the last state column an ordinary feature (`_free_last_column`), where seed 1030 + 65 is inside the bound (0.01 x).
  routed - 2900 rejected, 2901 in use. At 2900 the (hidden 256, B 17) case misses `actor m step 2` (117 x the bound): unit 202 of critic 1's second layer is 3.9e-8 of
    the layer's scale from zero at row 16 of the policy pass of the second update; the tile engine and the layer-at-a-time kernels (IL_GENERAL_TILES=0) agree with each
    other to the last bit shown and differ from the oracle in that one sample's contribution to the actor gradient. test_the_rejected_routed_base_is_a_relu_kink records
    the check, and that base 2901 has no such pre-activation in any back-propagated pass.
  dril - 2400, 2401, 2402 rejected, 2403 in use; each fails (B 3, H 254) alone, in the first update, with 3, 10 and 1 elements outside the tight bound (every element
    within one Adam step). All are weights of ONE saturated tanh unit (62, 221, 232) whose oracle gradients are 1e-9 .. 1e-7 - Adam's eps is 1e-8 - and the emulated
    kernel's are exactly half of the oracle's (2400, 2402) or exactly zero (2401): 1 - h * h of a saturated unit is a small multiple of 2^-24, and libm's tanhf and numpy's
    tanh differ there by one ulp of h. With three rows in the batch nothing else contributes to that unit's weights. This is the conditioning close_params documents, met
    with zero outliers allowed; it is not a ReLU kink, so no case is re-seeded for it - the family's base is simply the first at which all twelve cases pass.
Broken on purpose once, in a scratch copy: `if (row < n)` -> `if (row < Bp)` in k_g_pack (general.hip, the padding rows of the packed input) makes six cases of
test_general_actor_calls_at_edge_sizes fail on the emulated kernels (n1-H3, n1-H33, n2-H100, n17-H3, n17-H33, n33-H33: the BC step's parameters and loss).

Largest measured deviation / bound per family (`close`: |hip - oracle| over rtol |oracle| + atol; parameters: over the tight bound plus one Adam step per update): RECORDS
below, one set from the emulated kernels and one from the MI355X; the comment there says which cases have not been run on the GPU.
GMMIL with a single expert row is left out: n2 = 1 makes the median of the expert-to-expert distances 0 and gamma_2 = 1 / (0 + 1e-8), a bandwidth at which every kernel value
is 0 or 1 and a comparison says nothing."""
import atexit
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import inputs as gi
import test_dim_edges_gpu as G
import test_gpu_parity as P
from oracle import gail as ogail
from oracle import nets as onets
from oracle import sac as osac

pytestmark = pytest.mark.gpu

NARROW, WIDER, ONE = (11, 3), (17, 6), (1, 1)
SEEDS = dict(gail=2100, shaped=2200, deep=1010, shaped_deep=1030, red=2300, dril=2403, general=2500, actor=2600, fused=2700, bc=2800, routed=2901)

# family -> largest measured deviation over its bound, (emulated kernels, MI355X). Emulated: the module as it stands, without the one cell
# tests/test_size_edges_emulated.py leaves to the GPU. MI355X: the whole module (199 of 199 passed) BEFORE its last re-pairing; not run on the GPU since: DRIL at fixed
# base 2403 with the batches of 1 - 3 at hidden 66 / 254 / 256, the fused BC / acting body at hidden 192 and 256, the routed cases at base 2901, and the general-SAC cells
# (384, 3), (130, 64), (17, 144) and the depth-4 cells that were depth 8. GMMIL, PWIL and Adam / Polyak assert their siblings' bounds directly and are not listed.
RECORDS = {
    'plain GAIL': (0.12, 0.12), 'shaped GAIL': (0.41, 0.41), 'gail_deep': (0.11, 0.11), 'gail_shaped_deep': (0.035, 0.035),
    'RED': (0.092, 0.10), 'RED (parameters)': (6.3e-04, 5.8e-05), 'DRIL': (0.079, 0.045), 'DRIL (parameters)': (0.0044, 5.8e-05),
    'general SAC': (0.31, 0.69), 'general SAC (parameters)': (0.015, 0.12), 'general actor calls': (0.21, 0.26), 'general actor calls (parameters)': (0.042, 0.014),
    'fused SAC': (0.15, 0.15), 'fused BC and actor forward': (0.22, 0.17), 'fused BC and actor forward (parameters)': (2.7e-04, 1.1e-04),
    'fused shape, ragged batch': (0.12, 0.18), 'fused shape, ragged batch (parameters)': (0.010, 0.0068),
}

WORST = {}   # this run's figures, written to $IL_SIZE_EDGES_RECORD as JSON when the process ends


def _note(family, ratio):
  WORST[family] = max(WORST.get(family, 0.0), float(ratio))


@atexit.register
def _write_records():
  if os.environ.get('IL_SIZE_EDGES_RECORD') and WORST:
    with open(os.environ['IL_SIZE_EDGES_RECORD'], 'w') as f: json.dump(WORST, f, indent=1, sort_keys=True)


def close(family, a, b, name, rtol=1e-5, atol_scale=2e-6):
  x, y = np.asarray(a, np.float64), np.asarray(b, np.float64)
  if x.shape == y.shape and x.size: _note(family, (np.abs(x - y) / (rtol * np.abs(y) + atol_scale * max(float(np.abs(y).max()), 1e-30))).max())
  P.close(a, b, name, rtol=rtol, atol_scale=atol_scale)


def close_params(family, a, b, name, lr, steps=1):
  x, y = np.asarray(a, np.float64), np.asarray(b, np.float64)
  if x.shape == y.shape and x.size: _note(family + ' (parameters)', (np.abs(x - y) / (1e-5 * np.abs(y) + 1e-5 * max(float(np.abs(y).max()), 1e-30) + 1.01 * lr * steps)).max())
  P.close_params(a, b, name, lr, steps)   # (on a tensor of fewer than 2,000 elements its outlier fraction of 5e-4 means zero outliers)
  assert (np.abs(x - y) <= 1e-5 * np.abs(y) + 1e-5 * max(float(np.abs(y).max()), 1e-30)).all(), f'{name}: an element outside the tight bound (zero outliers are allowed here)'


def _pairs(batches, widths, shifts=(0, 3)):
  """(batch, width) pairs in which every batch and every width occurs at least len(shifts) times: the longer list once per shift, the shorter one cycled against it."""
  n = max(len(batches), len(widths))
  return sorted({(batches[i % len(batches)], widths[(i + s) % len(widths)]) for s in shifts for i in range(n)})


def _dims_for(i, batch, hidden):
  return ONE if batch == 1 and hidden in (1, 2) else (NARROW, WIDER)[i % 2]   # one case per family at (S, A) = (1, 1): its smallest batch and width


bh = lambda b, h: f'B{b}-H{h}'


# ------------------------------------------------------------------------------------------------ plain GAIL
GAIL_LOSSES = (('BCE', float('inf')), ('PUGAIL', float('inf')), ('PUGAIL', 0.02), ('Mixup', float('inf')))
GAIL_BATCHES = tuple(b for b in gi.EDGE_BATCHES if b <= 65)
GAIL_CASES = [pytest.param(b, h, *GAIL_LOSSES[i % 4], id=f'{bh(b, h)}-{GAIL_LOSSES[i % 4][0]}{"-margin" if GAIL_LOSSES[i % 4][1] == 0.02 else ""}')
              for i, (b, h) in enumerate(_pairs(GAIL_BATCHES, gi.EDGE_HIDDEN_GAIL, shifts=(0, 1, 2)))]


def _gail_body(dims, batch, hidden, loss, margin, seed, edit=None, reward_function='AIRL', reward_close=None, state_only_values=(False, True)):
  """The body of test_gail_ragged_batch_and_state_only (gradient, parameters and reward for both `state_only` values, the module's own initial parameters) with the loss
  variants of test_gail_loss_variants_match_reference / test_gail_pugail_finite_margin_matches_reference and their bounds.
  For tests/test_value_edges_gpu.py: `edit(case)` changes the finished inputs in place; `reward_close(family, got, want, name, logits, **bounds)` takes the place of
  `close` for the reward (the same bounds, applied per group of rows) and also sees the oracle's logits of the compared rows."""
  g = gi.gail_case(seed, env=dims, hidden=hidden, batch=batch, steps=1)
  eps_mix = gi.gail_extras(seed, g)['eps_mix'][0]
  G._free_last_column(dims, 2, g['policy'][0], g['expert'][0])
  if edit is not None: edit(g)
  torch.manual_seed(seed)
  grad_atol = 4e-6 if loss == 'BCE' or margin != float('inf') else 1e-5
  for state_only in state_only_values:
    icfg = P.Cfg(state_only=state_only, spectral_norm=True, loss_function=loss, grad_penalty=0.5, mixup_alpha=0.7, entropy_bonus=0.01, pos_class_prior=0.7, nonnegative_margin=margin,
                 discriminator=P.Cfg(hidden_size=hidden, depth=1, activation='relu', reward_shaping=False, subtract_log_policy=False, reward_function=reward_function))
    d = P.il.GAILDiscriminator(g['S'], g['A'], icfg, 0.97, device=P.DEV)
    D = g['S'] if state_only else g['D']
    ods = ogail.DiscState(D, hidden, True)
    ods.unpack_into(P.N(d.flat)); v = d.views()
    for k in ('u1', 'v1', 'u2', 'v2'):
      getattr(ods, k)[...] = P.N(v[k])
    opt = P.il.AdamW(d, lr=1e-4, weight_decay=1.0)
    pb, eb = g['policy'][0], g['expert'][0]
    cat = (lambda b: b['states']) if state_only else (lambda b: np.concatenate([b['states'], b['actions']], axis=1))
    P.il.adversarial_imitation_update(None, d, P.tbatch(pb), P.tbatch(eb), opt, icfg, eps_gp=P.T(g['eps'][0]), eps_mix=P.T(eps_mix) if loss == 'Mixup' else None)
    ogr = ogail.gail_update(ods, cat(pb), pb['weights'], cat(eb), eb['weights'], g['eps'][0], lr=1e-4, weight_decay=1.0, grad_penalty=0.5, entropy_bonus=0.01, return_grads=True,
                            loss_function=loss, pos_class_prior=0.7, nonnegative_margin=margin, eps_mix=eps_mix if loss == 'Mixup' else None)
    close('plain GAIL', P.N(opt.grad), ogr, f'disc grad (state_only={state_only})', atol_scale=grad_atol)
    close('plain GAIL', P.N(d.flat), ods.pack(), f'disc params (state_only={state_only})', atol_scale=4e-6)
    got, want = P.N(d.predict_reward(P.T(pb['states']), P.T(pb['actions']))), ogail.predict_reward(ods, cat(pb), reward_function)
    if reward_close is None: close('plain GAIL', got, want, 'reward', rtol=1e-4, atol_scale=1e-5)
    else: reward_close('plain GAIL', got, want, f'reward (state_only={state_only})', ogail.disc_logits(ods, cat(pb)), rtol=1e-4, atol_scale=1e-5)
    assert int(opt.step_count[0]) == 1   # (a PUGAIL value pass does not tick the optimiser)


@pytest.mark.parametrize('batch,hidden,loss,margin', GAIL_CASES)
def test_gail_discriminator_at_edge_sizes(batch, hidden, loss, margin):
  """il_gail_disc_step / il_gail_reward, hidden 16 (one k-block), 48, 240 and 512 (il_disc's limit: its LDS check admits it at S + A = 14 - 57 H + 916 floats), batches of
  1 .. 65 rows: BCE, PUGAIL with an infinite margin and with 0.02, Mixup."""
  i = GAIL_BATCHES.index(batch)
  _gail_body((NARROW, WIDER)[i % 2], batch, hidden, loss, margin, SEEDS['gail'] + batch + hidden)


def test_gail_discriminator_at_one_by_one():
  _gail_body(ONE, 1, 16, 'BCE', float('inf'), SEEDS['gail'] + 1)
  _gail_body(ONE, 3, 48, 'Mixup', float('inf'), SEEDS['gail'] + 3)


# ------------------------------------------------------------------------------------------------ reward-shaping GAIL
SHAPED_BATCHES = (1, 2, 3, 15, 17, 33, 65)
LOSSES3 = (('BCE', float('inf')), ('PUGAIL', float('inf')), ('Mixup', float('inf')), ('PUGAIL', 0.02))
SHAPED_CASES = [pytest.param(b, h, *LOSSES3[i % 4], id=f'{bh(b, h)}-{LOSSES3[i % 4][0]}{"-margin" if LOSSES3[i % 4][1] == 0.02 else ""}')
                for i, (b, h) in enumerate(_pairs(SHAPED_BATCHES, gi.EDGE_HIDDEN_SHAPED))]


@pytest.mark.parametrize('batch,hidden,loss,margin', SHAPED_CASES)
def test_shaped_gail_at_edge_sizes(batch, hidden, loss, margin):
  """il_gail_shaped_step / il_gail_shaped_reward (the body of test_shaped_gail_at_edge_widths, its bounds): the gradient of one update and the GAIL-head reward with a
  potential of 1 .. 256 hidden units at batches of 1 .. 65 rows with fractional terminals."""
  i = SHAPED_BATCHES.index(batch)
  _shaped_body(_dims_for(i, batch, hidden), batch, hidden, loss, margin, SEEDS['shaped'] + batch + hidden)


def _shaped_body(dims, batch, hidden, loss, margin, seed, edit=None, reward_function='GAIL', reward_close=None):
  """The body of test_shaped_gail_at_edge_sizes; `edit`, `reward_function` and `reward_close` as in _gail_body."""
  from oracle import gail_shaped as ogs
  c = gi.gail_shaped_case(seed, dims, hidden, batch, 1, True)
  em = gi.mixup_draws(seed + 1000, batch, 1)[0]
  G._free_last_column(dims, 5, c['policy'][0], c['expert'][0])
  if edit is not None: edit(c)
  icfg = P.Cfg(state_only=False, spectral_norm=True, loss_function=loss, grad_penalty=1.0, mixup_alpha=0.7, entropy_bonus=0.0, pos_class_prior=0.7, nonnegative_margin=margin,
               discriminator=P.Cfg(hidden_size=hidden, depth=1, activation='relu', reward_shaping=True, subtract_log_policy=False, reward_function=reward_function))
  dd = P.il.GAILDiscriminator(c['S'], c['A'], icfg, 0.99, device=P.DEV)
  assert type(dd).__name__ == 'ShapedGAILDiscriminator'
  ods = ogs.ShapedState(c['S'], c['A'], hidden, 0.99, True)
  for k in ('Wg', 'bg', 'W1', 'b1', 'W2', 'b2', 'ug', 'vg', 'u1', 'v1', 'u2', 'v2'):
    getattr(ods, k)[...] = c[k]
  dd.flat.copy_(P.T(ods.pack()))
  for k, v in dd.views().items():
    v.copy_(P.T(c[k]))
  opt = P.il.AdamW(dd, lr=1e-3, weight_decay=0.0)
  P.il.adversarial_imitation_update(None, dd, P.tbatch(c['policy'][0]), P.tbatch(c['expert'][0]), opt, icfg, eps_gp=P.T(c['eps'][0]), eps_mix=P.T(em) if loss == 'Mixup' else None)
  og = ogs.gail_update(ods, c['policy'][0], c['expert'][0], c['eps'][0], lr=1e-3, weight_decay=0.0, grad_penalty=1.0, return_grads=True, loss_function=loss, pos_class_prior=0.7,
                       nonnegative_margin=margin, eps_mix=em if loss == 'Mixup' else None)
  close('shaped GAIL', P.N(opt.grad), og, 'shaped GAIL gradient', rtol=1e-5, atol_scale=1e-5)
  p = P.tbatch(c['policy'][0])
  dd.flat.copy_(P.T(ods.pack()))
  got, want = P.N(dd.predict_reward(p['states'], p['actions'], p['next_states'], p['terminals'])), ogs.predict_reward(ods, c['policy'][0], reward_function)
  if reward_close is None: close('shaped GAIL', got, want, 'shaped GAIL reward', rtol=2e-5, atol_scale=1e-5)
  else: reward_close('shaped GAIL', got, want, 'shaped GAIL reward', ogs.forward(ods, *ogs._split(ods, c['policy'][0])[:4])[0], rtol=2e-5, atol_scale=1e-5)
  assert int(opt.step_count[0]) == 1


# ------------------------------------------------------------------------------------------------ the general discriminators
DEEP_NETS = ((2, 'tanh'), (1, 'relu'), (2, 'relu'), (1, 'tanh'))
DEEP_LOSSES = ('BCE', 'PUGAIL', 'Mixup')
DEEP_CELLS = _pairs(SHAPED_BATCHES, gi.EDGE_HIDDEN_DEEP) + [(65, 128)]   # (65, 128): the cell of the known ReLU kink (module docstring), beside the paired ones
DEEP_CASES = [pytest.param(b, h, *DEEP_NETS[i % 4], DEEP_LOSSES[(i // 4 + i) % 3], id=f'{bh(b, h)}-d{DEEP_NETS[i % 4][0]}-{DEEP_NETS[i % 4][1]}-{DEEP_LOSSES[(i // 4 + i) % 3]}')
              for i, (b, h) in enumerate(DEEP_CELLS)]
SHAPED_DEEP_CASES = [c for c in DEEP_CASES if c.values[:2] != (65, 128)] + [pytest.param(65, 128, 1, 'relu', 'BCE', id='B65-H128-d1-relu-BCE')]


@pytest.mark.parametrize('batch,hidden,depth,activation,loss', DEEP_CASES)
def test_gail_deep_at_edge_sizes(batch, hidden, depth, activation, loss):
  """gail_deep.hip against oracle/gail_deep.py (the body and bounds of test_gail_deep_at_edge_widths): the gradient and the spectral-norm buffers of one update with gradient
  penalty and entropy bonus, the AIRL reward on the oracle's updated parameters; hidden 2 .. 128, batches of 1 .. 65 rows."""
  _deep_body(_dims_for(SHAPED_BATCHES.index(batch), batch, hidden), batch, hidden, depth, activation, loss, SEEDS['deep'] + batch)


def _deep_body(dims, batch, hidden, depth, activation, loss, seed, edit=None, reward_function='AIRL', reward_close=None):
  """The body of test_gail_deep_at_edge_sizes; `edit`, `reward_function` and `reward_close` as in _gail_body."""
  from oracle import gail_deep as ogd
  lr, wd, gp, ent = 1e-3, 0.1, 0.6, 0.02
  c = gi.gail_deep_case(seed=seed, env=dims, hidden=hidden, batch=batch, steps=1, depth=depth, activation=activation, spectral_norm=True)
  G._free_last_column(dims, 6, c['policy'][0], c['expert'][0])
  if edit is not None: edit(c)
  icfg = P.Cfg(state_only=False, spectral_norm=True, loss_function=loss, grad_penalty=gp, mixup_alpha=0.7, entropy_bonus=ent, pos_class_prior=0.7, nonnegative_margin=float('inf'),
               discriminator=P.Cfg(hidden_size=hidden, depth=depth, activation=activation, reward_shaping=False, subtract_log_policy=False, reward_function=reward_function))
  d = P.il.models.DeepGAILDiscriminator(c['S'], c['A'], icfg, 0.97, device=P.DEV)
  ds = ogd.DeepDiscState(c['D'], hidden, depth, activation, True)
  for l in range(depth + 1):
    ds.W[l][...] = c['W'][l]; ds.b[l][...] = c['b'][l]; ds.u[l][...] = c['u'][l]; ds.v[l][...] = c['v'][l]
  d.flat.copy_(P.T(ds.pack())); d.sn.copy_(P.T(ds.pack_sn()))
  opt = P.il.AdamW(d, lr=lr, weight_decay=wd)
  cat = lambda b: np.concatenate([b['states'], b['actions']], 1)
  pb, eb = c['policy'][0], c['expert'][0]
  P.il.adversarial_imitation_update(None, d, P.tbatch(pb), P.tbatch(eb), opt, icfg, eps_gp=P.T(c['eps'][0]), eps_mix=P.T(c['eps_mix'][0]))
  ogr = ogd.gail_update(ds, cat(pb), pb['weights'], cat(eb), eb['weights'], c['eps'][0], lr=lr, weight_decay=wd, grad_penalty=gp, entropy_bonus=ent, return_grads=True, loss_function=loss,
                        pos_class_prior=0.7, eps_mix=c['eps_mix'][0])
  close('gail_deep', P.N(opt.grad), ogr, 'deep gradient', rtol=2e-5, atol_scale=1e-5)
  close('gail_deep', P.N(d.sn), ds.pack_sn(), 'deep u / v', rtol=2e-5, atol_scale=1e-5)
  d.flat.copy_(P.T(ds.pack()))
  got, want = P.N(d.predict_reward(P.T(pb['states']), P.T(pb['actions']))), ogd.predict_reward(ds, cat(pb), reward_function)
  if reward_close is None: close('gail_deep', got, want, 'deep reward', rtol=5e-5, atol_scale=1e-5)
  else: reward_close('gail_deep', got, want, 'deep reward', ogd.disc_logits(ds, cat(pb)), rtol=5e-5, atol_scale=1e-5)
  assert int(opt.step_count[0]) == 1


def _shaped_deep_case(batch, hidden, depth, activation):
  dims = _dims_for(SHAPED_BATCHES.index(batch), batch, hidden)
  c = gi.gail_shaped_deep_case(seed=SEEDS['shaped_deep'] + batch, env=dims, hidden=hidden, batch=batch, steps=1, depth=depth, activation=activation, spectral_norm=True)
  G._free_last_column(dims, 6, c['policy'][0], c['expert'][0])
  return c


@pytest.mark.parametrize('batch,hidden,depth,activation,loss', SHAPED_DEEP_CASES)
def test_gail_shaped_deep_at_edge_sizes(batch, hidden, depth, activation, loss):
  """gail_shaped_deep.hip against oracle/gail_shaped_deep.py (the body and bounds of test_gail_shaped_deep_at_edge_widths): gradient, u / v, the AIRL reward; a potential of
  2 .. 128 hidden units, batches of 1 .. 65 rows with fractional terminals."""
  _shaped_deep_body(_shaped_deep_case(batch, hidden, depth, activation), hidden, depth, activation, loss)


def _shaped_deep_body(c, hidden, depth, activation, loss, reward_function='AIRL', reward_close=None):
  """The body of test_gail_shaped_deep_at_edge_sizes on a prepared case; `reward_function` and `reward_close` as in _gail_body."""
  from oracle import gail_shaped_deep as osd
  from test_oracle_golden import _shaped_deep_state
  lr, wd, gp, ent = 1e-3, 0.1, 0.7, 0.01
  icfg = P.Cfg(state_only=False, spectral_norm=True, loss_function=loss, grad_penalty=gp, mixup_alpha=0.7, entropy_bonus=ent, pos_class_prior=0.7, nonnegative_margin=float('inf'),
               discriminator=P.Cfg(hidden_size=hidden, depth=depth, activation=activation, reward_shaping=True, subtract_log_policy=False, reward_function=reward_function))
  d = P.il.models.ShapedDeepGAILDiscriminator(c['S'], c['A'], icfg, 0.97, device=P.DEV)
  ods = _shaped_deep_state(c)
  d.flat.copy_(P.T(ods.pack())); d.sn.copy_(P.T(ods.pack_sn()))
  opt = P.il.AdamW(d, lr=lr, weight_decay=wd)
  pb, eb = c['policy'][0], c['expert'][0]
  P.il.adversarial_imitation_update(None, d, P.tbatch(pb), P.tbatch(eb), opt, icfg, eps_gp=P.T(c['eps'][0]), eps_mix=P.T(c['eps_mix'][0]))
  ogr = osd.gail_update(ods, pb, eb, c['eps'][0], lr=lr, weight_decay=wd, grad_penalty=gp, entropy_bonus=ent, return_grads=True, loss_function=loss, pos_class_prior=0.7,
                        nonnegative_margin=float('inf'), eps_mix=c['eps_mix'][0])
  close('gail_shaped_deep', P.N(opt.grad), ogr, 'shaped deep gradient', rtol=2e-5, atol_scale=1e-5)
  close('gail_shaped_deep', P.N(d.sn), ods.pack_sn(), 'shaped deep u / v', rtol=2e-5, atol_scale=1e-5)
  d.flat.copy_(P.T(ods.pack()))
  p = P.tbatch(pb)
  r = d.predict_reward(**P.il.make_gail_input(p['states'], p['actions'], p['next_states'], p['terminals'], None, True, False))
  want = osd.predict_reward(ods, pb, reward_function)
  if reward_close is None: close('gail_shaped_deep', P.N(r), want, 'shaped deep reward', rtol=5e-5, atol_scale=1e-5)
  else: reward_close('gail_shaped_deep', P.N(r), want, 'shaped deep reward', osd.forward(ods, *osd._split(ods, pb)[:4])[0], rtol=5e-5, atol_scale=1e-5)
  assert int(opt.step_count[0]) == 1


def _kink_units(c, hyper=(1e-3, 0.1, 0.7, 0.01)):
  """Hidden units of a depth-1 ReLU potential whose pre-activation is within 1e-6 of the layer's scale of zero at some row of some forward of the ORACLE's update: its
  `_forward` is wrapped while `gail_update` runs, so the rows (policy, expert, the gradient penalty's mixture; states and next states) and the spectrally normalised
  weights (one more power iteration per use) are the oracle's own, in float32. Returns {unit: smallest |z| / max |z| of its layer}."""
  from oracle import gail_shaped_deep as osd
  from test_oracle_golden import _shaped_deep_state
  lr, wd, gp, ent = hyper
  seen, real = {}, osd._forward

  def recording(Wh, b, x, act):
    z = (x.astype(np.float32) @ Wh[0].T + b[0]).astype(np.float32)
    rel = np.abs(z).min(axis=0) / np.abs(z).max()
    for unit in np.nonzero(rel <= 1e-6)[0].tolist():
      seen[unit] = min(seen.get(unit, 1.0), float(rel[unit]))
    return real(Wh, b, x, act)
  osd._forward = recording
  try:
    osd.gail_update(_shaped_deep_state(c), c['policy'][0], c['expert'][0], c['eps'][0], lr=lr, weight_decay=wd, grad_penalty=gp, entropy_bonus=ent, loss_function='BCE', pos_class_prior=0.7,
                    nonnegative_margin=float('inf'), eps_mix=c['eps_mix'][0])
  finally:
    osd._forward = real
  return seen


def test_the_rejected_shaped_deep_seed_is_a_relu_kink():
  """The rejected seed (1030 + 65) of the (B 65, H 128, depth 1, relu) cell at (11, 3) with the builder's absorbing column: the flat gradient is g.bias [1], g.weight [14],
  h.0.bias [128], h.0.weight [128][11], h.2.bias [1], h.2.weight [128] (`named_parameters` order with spectral norm: bias before the parametrised weight). The deviating
  elements - 24 = h.0.bias[9], 242 .. 251 = h.0.weight[9, 0:10] (column 10 is the absorbing bit, zero in every row that matters) - all belong to hidden unit 9, and unit 9
  has a pre-activation within 1e-6 of the layer's scale of zero in the oracle's own forward. No kernel runs here: this is the record of why that seed was rejected."""
  dims = NARROW
  c = gi.gail_shaped_deep_case(seed=1030 + 65, env=dims, hidden=128, batch=65, steps=1, depth=1, activation='relu', spectral_norm=True)
  units = _kink_units(c)
  S, A, H = c['S'], c['A'], 128
  o_b1 = 1 + (S + A)
  o_W1, o_W2 = o_b1 + H, o_b1 + H + H * S + 1
  owners = set()
  for i in [24] + list(range(242, 252)):
    if o_b1 <= i < o_W1: owners.add(i - o_b1)
    elif o_W1 <= i < o_W1 + H * S: owners.add((i - o_W1) // S)
    elif o_W2 <= i < o_W2 + H: owners.add(i - o_W2)
    else: owners.add(('not a hidden unit', i))
  assert owners == {9} and owners <= set(units), (owners, units)


# ------------------------------------------------------------------------------------------------ RED, DRIL
RED_BATCHES = (1, 2, 3, 17, 33, 65)
RED_CASES = [pytest.param(b, h, id=bh(b, h)) for b, h in _pairs(RED_BATCHES, gi.EDGE_HIDDEN_RED, shifts=(0, 2))]


def _red_body(dims, batch, hidden, edit=None):
  from oracle import red as ored
  c = gi.red_case(SEEDS['red'] + batch + hidden, dims, hidden, batch, 2)
  G._free_last_column(dims, 3, *c['batches'], c['query'])
  if edit is not None: edit(c)   # (tests/test_value_edges_gpu.py: changes the finished inputs in place)
  icfg = P.Cfg(state_only=False, reward_bandwidth_scale=None, discriminator=P.Cfg(hidden_size=hidden, depth=1, activation='relu', input_dropout=0, dropout=0))
  d = P.il.REDDiscriminator(c['S'], c['A'], icfg, device=P.DEV)
  d.flat.copy_(P.T(c['predictor'])); d.target_flat.copy_(P.T(c['target']))
  opt = P.il.AdamW(d, lr=1e-3, weight_decay=0.0)
  st = ored.RedState(c['D'], c['H']); st.predictor[:] = c['predictor']; st.target[:] = c['target']
  for k, b in enumerate(c['batches'], 1):
    P.il.target_estimation_update(d, P.tbatch(b), opt)
    ored.target_estimation_update(st, np.concatenate([b['states'], b['actions']], 1), b['weights'], lr=1e-3, weight_decay=0.0)
    close_params('RED', P.N(d.flat), st.predictor, f'size edge {bh(batch, hidden)} RED predictor {k}', 1e-3, steps=k)
  d.flat.copy_(P.T(st.predictor)); d.eval()
  q = c['query']
  x = np.concatenate([q['states'], q['actions']], 1)
  for n in (1, batch + 16):
    pred, targ = d(P.T(q['states'][:n]), P.T(q['actions'][:n]))
    op, ot, _ = ored.forward(st, x[:n])
    close('RED', P.N(pred), op, f'predictor embedding n={n}'); close('RED', P.N(targ), ot, f'target embedding n={n}')


@pytest.mark.parametrize('batch,hidden', RED_CASES)
def test_red_at_edge_sizes(batch, hidden):
  """il_red_step (the body of test_red_at_edge_widths): two updates, zero outliers; then il_red_forward in eval mode on a query of 1 and of B + 16 rows (the bound of
  test_red_matches_reference's embeddings). Even widths 2 .. 256, batches of 1 .. 65 rows."""
  _red_body((NARROW, WIDER)[RED_BATCHES.index(batch) % 2], batch, hidden)


def _dril_body(dims, batch, hidden, edit=None, after_step=None):
  from oracle import dril as odril
  c = gi.dril_case(SEEDS['dril'] + batch + hidden, dims, hidden, batch, 2)
  G._free_last_column(dims, 4, *c['batches'], c['query'])
  if edit is not None: edit(c)   # (tests/test_value_edges_gpu.py: changes the finished inputs in place)
  a = P.il.SoftActor(c['S'], c['A'], P.Cfg(hidden_size=hidden, depth=1, activation='tanh', input_dropout=0.1, dropout=0.1), device=P.DEV)
  a.flat.copy_(P.T(c['params']))
  opt = P.il.AdamW(a, lr=1e-3, weight_decay=0.0)
  ds = odril.DrilState(c['S'], c['A'], hidden, 0.1, 0.1); ds.params[:] = c['params']
  for k, (b, m0, m1) in enumerate(zip(c['batches'], c['m0'], c['m1']), 1):
    P.il.behavioural_cloning_update(a, P.tbatch(b), opt, masks=(P.T(m0), P.T(m1)))
    odril.bc_update(ds, b, m0, m1, lr=1e-3, weight_decay=0.0)
    close_params('DRIL', P.N(a.flat), ds.params, f'size edge {bh(batch, hidden)} DRIL params {k}', 1e-3, steps=k)
    if after_step is not None: after_step(k, P.N(opt.exp_avg), ds.m)   # (tests/test_value_edges_gpu.py: further comparisons, per slab of the parameter vector)
  q = P.tbatch(c['query'])
  ou = odril.uncertainty(ds, c['query']['states'], c['query']['actions'], c['q_m0'], c['q_m1'])
  a.flat.copy_(P.T(ds.params)); u = P.N(a._get_action_uncertainty(q['states'], q['actions'], masks=(P.T(c['q_m0']), P.T(c['q_m1']))))
  _note('DRIL', np.abs(u - ou).max() / (1e-4 * max(np.abs(ou).max(), 1e-30)))
  assert np.abs(u - ou).max() <= 1e-4 * max(np.abs(ou).max(), 1e-30)


@pytest.mark.parametrize('batch,hidden', RED_CASES)
def test_dril_at_edge_sizes(batch, hidden):
  """il_dril (the body of test_dril_at_edge_widths): two updates with given dropout masks, zero outliers, then the Monte-Carlo uncertainty of the query set. A batch of
  one row among them (tests/golden/inputs.py dril_case clamps its "exercise the clamp" rows to the rows there are)."""
  _dril_body((NARROW, WIDER)[RED_BATCHES.index(batch) % 2], batch, hidden)


def test_red_and_dril_at_one_by_one():
  """(S, A) = (1, 1): an input of two columns (RED) and of one (DRIL), at a batch of 3 and hidden 6."""
  _red_body(ONE, 3, 6); _dril_body(ONE, 3, 6)


# ------------------------------------------------------------------------------------------------ SAC through csrc/general.hip
def _sac_updates(family, c, dims, steps=2, what='general'):
  """`steps` sac_update calls against osac.sac_update (the loop of test_general_shape_sac_matches_oracle_and_reference, its bounds): log pi, Q, actor, critics, target,
  log alpha, the Adam first moments."""
  G._free_last_column(dims, c['B'], *c['batches'])
  actor, critic, target, log_alpha, ao, co, to = P.make_sac(c)
  st = P.make_sac_oracle(c)
  for k in range(1, steps + 1):
    b = c['batches'][k - 1]
    logp, q = P.il.sac_update(actor, critic, log_alpha, target, P.tbatch(b), ao, co, to, c['discount'], c['entropy_target'], c['polyak'], eps_next=P.T(c['eps_next'][k - 1]), eps_cur=P.T(c['eps_cur'][k - 1]))
    ologp, oq = osac.sac_update(st, b, c['eps_next'][k - 1], c['eps_cur'][k - 1], discount=c['discount'], entropy_target=c['entropy_target'], polyak_factor=c['polyak'], lr=c['lr'], weight_decay=c['weight_decay'])
    torch.cuda.synchronize()
    close(family, P.N(logp), ologp, f'logp step {k}', atol_scale=2e-6 * k); close(family, P.N(q), oq, f'q step {k}', atol_scale=2e-6 * k)
    P.close_params(P.N(actor.flat), st.actor, f'size edge {what} actor step {k}', c['lr'], k); P.close_params(P.crit_from_flat(critic, critic.flat), st.critic, f'size edge {what} critic step {k}', c['lr'], k)
    P.close_params(P.crit_from_flat(critic, target.flat), st.target, f'size edge {what} target step {k}', c['lr'], k); close(family, P.N(log_alpha), st.log_alpha, f'log_alpha step {k}')
    for name, got, want in (('actor', P.N(actor.flat), st.actor), ('critic', P.crit_from_flat(critic, critic.flat), st.critic), ('target', P.crit_from_flat(critic, target.flat), st.target)):
      _note(family + ' (parameters)', (np.abs(got.astype(np.float64) - want) / (1e-5 * np.abs(want) + 1e-5 * np.abs(want).max() + 1.01 * c['lr'] * k)).max())
    close(family, P.N(ao.exp_avg), st.actor_m, f'actor m step {k}', atol_scale=1e-5 * k); close(family, P.crit_from_flat(critic, co.exp_avg), st.critic_m, f'critic m step {k}', atol_scale=1e-5 * k)
  assert int(ao.step_count[0]) == steps and int(co.step_count[0]) == steps and int(to.step_count[0]) == steps
  return actor, critic


GENERAL_BATCHES = gi.EDGE_BATCHES + (384,)
GENERAL_DEPTHS, GENERAL_ACTS, GENERAL_ENVS = (2, 1, 3, 4, 8), ('relu', 'tanh', 'sigmoid'), ('hopper', NARROW, 'wide', ONE)


def _general_cases():
  out, n = [], 0
  for i, b in enumerate(GENERAL_BATCHES):
    for shift in (0, 4):
      h = gi.EDGE_HIDDEN_GENERAL[(i + shift) % len(gi.EDGE_HIDDEN_GENERAL)]
      if (b, h) == (384, 127): h = 3   # the largest batch at the narrow widths (3 and 33); 127 keeps the batches of 15 and 63
      depth = GENERAL_DEPTHS[n % 5]
      if depth == 8 and h > 33 and (b, h) != (17, 257): depth = 4   # eight layers at hidden 1 .. 33 (B = 384 among them) and once at hidden 257
      out.append((b, h, depth, GENERAL_ACTS[n % 3], GENERAL_ENVS[n % 4], None)); n += 1
  # reinforcement.actor != reinforcement.critic, each way round: a wide actor beside narrow critics, and the reverse
  out += [(33, 100, 2, 'tanh', 'hopper', (3, 1, 'relu')), (15, 3, 1, 'relu', NARROW, (127, 3, 'sigmoid'))]
  # the tile engine (hidden a multiple of 16) at ragged batches: 127 pads to 128 rows, where the optimiser launches take the 32 x 32 block jobs with a padded row;
  # 64 wide hidden layers of depth 3 run from their lane-ordered copies
  out += [(127, 48, 3, 'tanh', NARROW, None), (129, 80, 1, 'sigmoid', 'hopper', None), (1, 16, 2, 'tanh', ONE, None), (3, 64, 3, 'relu', NARROW, None), (130, 64, 3, 'tanh', 'hopper', None),
          (17, 144, 2, 'relu', NARROW, None), (127, 64, 2, 'sigmoid', 'wide', (128, 1, 'tanh'))]
  env_id = lambda e: e if isinstance(e, str) else f'S{e[0]}A{e[1]}'
  return [pytest.param(*c, id=f'{bh(c[0], c[1])}-d{c[2]}-{c[3]}-{env_id(c[4])}' + (f'-critic{c[5][0]}d{c[5][1]}{c[5][2]}' if c[5] else '')) for c in out]


@pytest.mark.parametrize('batch,hidden,depth,activation,env,critic', _general_cases())
def test_general_sac_update_at_edge_sizes(batch, hidden, depth, activation, env, critic):
  """il_sac_update_general, two updates: hidden 1 .. 257 (the layer-at-a-time kernels), depths 1 .. 8, relu / tanh / sigmoid, batches of 1 .. 384 rows, the reference's
  hopper and the wide action space, (11, 3) and (1, 1); mixed actor / critic shapes both ways; and the tile engine (hidden a multiple of 16) at ragged batches."""
  kw = dict(seed=SEEDS['general'] + batch + hidden, env=env, hidden=hidden, batch=batch, steps=2, depth=depth, activation=activation)
  if critic is not None: kw['critic'] = critic
  c = gi.sac_case(**kw)
  actor, critic_net = _sac_updates('general SAC', c, env if not isinstance(env, str) else (0, 0))
  assert actor.general or critic_net.general


ACTOR_NS = (1, 2, 3, 15, 17, 33)
ACTOR_CASES = [pytest.param(n, h, GENERAL_DEPTHS[i % 4], GENERAL_ACTS[i % 3], id=f'n{n}-H{h}-d{GENERAL_DEPTHS[i % 4]}-{GENERAL_ACTS[i % 3]}')
               for i, (n, h) in enumerate(_pairs(ACTOR_NS, gi.EDGE_HIDDEN_GENERAL_ACTOR, shifts=(0, 1)))]


def _actor_calls(family, c, dims, ns, general, after_step=None):
  """Acting (a sample with fed noise, its log-probability, the greedy action), log pi of given actions and two behavioural_cloning_update steps against oracle/nets.py
  and osac.bc_update: the bounds of test_general_shape_sac_matches_oracle_and_reference's acting part (general) / of test_bc_and_actor_forward_at_edge_widths (fused)."""
  S, A, H, depth, act = c['S'], c['A'], c['H'], c['depth'], c['activation']
  G._free_last_column(dims, c['B'] + 1, *c['batches'])
  actor = P.make_sac(c)[0]
  assert actor.general == general
  shapes = onets.mlp_shapes(S, H, depth, 2 * A)
  b0 = c['batches'][0]
  tol = 2e-6 if general else 4e-6
  lp_tol = dict(rtol=1e-4, atol_scale=1e-5) if general else dict(atol_scale=4e-6)

  def head(s):
    out, _ = onets.mlp_forward(onets.unpack(c['actor'], shapes), s, activation=act)
    mean, _, _, std = onets.actor_head(out, A)
    return mean, std
  for n in ns:
    s, eps = b0['states'][:n], c['eps_cur'][0][:n]
    mean, std = head(s)
    x = mean + eps * std
    a, lp = actor(P.T(s)).sample_with_log_prob(P.T(eps))
    close(family, P.N(a), np.tanh(x), f'act sample n={n}', atol_scale=tol); close(family, P.N(lp), onets.tanh_gaussian_logp(x, mean, std), f'act logp n={n}', **lp_tol)
    close(family, P.N(actor.get_greedy_action(P.T(s))), np.tanh(mean), f'greedy n={n}', atol_scale=tol)
    xa = np.arctanh(np.clip(b0['actions'][:n], np.float32(-1 + 1e-6), np.float32(1 - 1e-6)).astype(np.float64))
    want = onets.tanh_gaussian_logp(xa.astype(np.float32), mean, std)
    close(family, P.N(actor.log_prob(P.T(s), P.T(b0['actions'][:n]))), want, f'log pi of given actions n={n}', rtol=1e-4, atol_scale=1e-5)
  p = c['actor'].copy()
  opt = P.il.AdamW(actor, lr=2.5e-4, weight_decay=0.01)
  m, v = np.zeros_like(p), np.zeros_like(p)
  for k in (1, 2):
    b = c['batches'][k - 1]
    loss = P.il.behavioural_cloning_update(actor, P.tbatch(b), opt)
    oloss = osac.bc_update(p, m, v, k, shapes, A, b, lr=2.5e-4, weight_decay=0.01, activation=act)
    close(family, P.N(loss), oloss, f'bc loss {k}', rtol=1e-5, atol_scale=1e-5)
    P.close_params(P.N(actor.flat), p, f'size edge {family} bc actor {k}', 2.5e-4, k); close(family, P.N(opt.exp_avg), m, f'bc m {k}', atol_scale=1e-5 * k)
    _note(family + ' (parameters)', (np.abs(P.N(actor.flat).astype(np.float64) - p) / (1e-5 * np.abs(p) + 1e-5 * np.abs(p).max() + 1.01 * 2.5e-4 * k)).max())
    if after_step is not None: after_step(k, P.N(opt.exp_avg), m)   # (tests/test_value_edges_gpu.py: further comparisons, per slab of the parameter vector)
  return actor


@pytest.mark.parametrize('n,hidden,depth,activation', ACTOR_CASES)
def test_general_actor_calls_at_edge_sizes(n, hidden, depth, activation):
  """il_actor_act_general, il_actor_log_prob_general and il_bc_step_general on n = 1 .. 33 rows, hidden 3 .. 257."""
  dims = (NARROW, WIDER)[ACTOR_NS.index(n) % 2]
  c = gi.sac_case(SEEDS['actor'] + n + hidden, dims, hidden, n, 2, depth=depth, activation=activation)
  _actor_calls('general actor calls', c, dims, (n,), True)


def test_general_sac_and_actor_calls_at_one_by_one():
  c = gi.sac_case(SEEDS['actor'] + 1, ONE, 3, 2, 2, depth=1, activation='tanh')
  _actor_calls('general actor calls', c, ONE, (1, 2), True)


# ------------------------------------------------------------------------------------------------ the fused SAC kernels
FUSED_BATCHES = (48, 80, 112, 144, 272)
# every batch twice, every width twice (64 and 128 three times); the two largest batches at the two narrower widths (the emulated run pays per MFMA)
FUSED_PAIRS = ((48, 192), (48, 256), (80, 128), (80, 256), (112, 64), (112, 192), (144, 64), (144, 128), (272, 64), (272, 128))
FUSED_CASES = [pytest.param(b, h, id=bh(b, h)) for b, h in FUSED_PAIRS]


@pytest.mark.parametrize('batch,hidden,dims', [pytest.param(b, h, (NARROW, WIDER)[FUSED_BATCHES.index(b) % 2], id=bh(b, h)) for b, h in FUSED_PAIRS]
                         + [pytest.param(48, 64, ONE, id='B48-H64-S1A1')])
def test_fused_sac_update_at_edge_sizes(batch, hidden, dims):
  """One fused `il.sac_update` against `osac.sac_update` (the body and bounds of test_sac_update_at_edge_widths) at 3, 5, 7, 9 and 17 row tiles."""
  _fused_sac_body(gi.sac_case(SEEDS['fused'] + batch + hidden, dims, hidden, batch, 1), dims, batch, hidden)


def _fused_sac_body(c, dims, batch, hidden):
  """The body of test_fused_sac_update_at_edge_sizes on a prepared case."""
  G._free_last_column(dims, batch, *c['batches'])
  actor, critic, target, log_alpha, ao, co, to = P.make_sac(c)
  assert not actor.general and not critic.general
  st = P.make_sac_oracle(c)
  b = c['batches'][0]
  logp, q = P.il.sac_update(actor, critic, log_alpha, target, P.tbatch(b), ao, co, to, c['discount'], c['entropy_target'], c['polyak'], eps_next=P.T(c['eps_next'][0]), eps_cur=P.T(c['eps_cur'][0]))
  ologp, oq = osac.sac_update(st, b, c['eps_next'][0], c['eps_cur'][0], discount=c['discount'], entropy_target=c['entropy_target'], polyak_factor=c['polyak'], lr=c['lr'])
  close('fused SAC', P.N(logp), ologp, 'logp', atol_scale=4e-6); close('fused SAC', P.N(q), oq, 'q', atol_scale=4e-6)
  P.close_params(P.N(actor.flat), st.actor, f'size edge {bh(batch, hidden)} actor', c['lr']); P.close_params(P.crit_from_flat(critic, critic.flat), st.critic, f'size edge {bh(batch, hidden)} critic', c['lr'])
  P.close_params(P.crit_from_flat(critic, target.flat), st.target, f'size edge {bh(batch, hidden)} target', c['lr']); close('fused SAC', P.N(log_alpha), st.log_alpha, 'log_alpha')


@pytest.mark.parametrize('batch,hidden', FUSED_CASES)
def test_fused_bc_and_actor_forward_at_edge_sizes(batch, hidden):
  """il_actor_act and il_actor_log_prob on n = 1, 2, 3, 15, 17, 31, 33 rows and two il_bc_step updates (the body and bounds of test_bc_and_actor_forward_at_edge_widths)."""
  dims = (NARROW, WIDER)[FUSED_BATCHES.index(batch) % 2]
  c = gi.sac_case(SEEDS['bc'] + batch + hidden, dims, hidden, batch, 2)
  _actor_calls('fused BC and actor forward', c, dims, (1, 2, 3, 15, 17, 31, 33), False)


# ------------------------------------------------------------------------------------------------ fused-shape networks at a batch that is not whole 16-row tiles
@pytest.mark.parametrize('batch', [100, 17])
@pytest.mark.parametrize('hidden', [128, 256])
def test_fused_shape_sac_update_at_a_ragged_batch_runs_the_general_kernels(batch, hidden):
  """train.py's per-function path at `training.batch_size=100`: `il.sac_update` with the default (fused-shape: depth 2, relu, hidden 128 / 256) networks and B % 16 != 0
  used to stop with il_sac's `batch=100 must be a positive multiple of 16`; it now runs csrc/general.hip (same parameter layout). Two steps against osac.sac_update."""
  c = gi.sac_case(SEEDS['routed'] + batch + hidden, NARROW, hidden, batch, 2)
  actor, critic = _sac_updates('fused shape, ragged batch', c, NARROW, what='routed')
  assert not actor.general and not critic.general


def _relu_kinks(c, steps=2, rel=1e-6):
  """(update, pass, layer, row, unit, |z| / max |z|) of every ReLU pre-activation within `rel` of its layer's scale of zero in the oracle's own float32 forwards of the
  three back-propagated passes (critics on (s, a), actor on s, critics on (s, a~): calls 4 .. 8 of nets.mlp_forward within osac.sac_update) of `steps` updates."""
  st, found, real, calls = P.make_sac_oracle(c), [], onets.mlp_forward, []

  def recording(layers, x, masks=None, activation='relu'):
    calls.append(0)
    if len(calls) > 3:   # (the first three forwards - actor and targets on s' - carry no gradient)
      h = x.astype(np.float32)
      for li, (W, b) in enumerate(layers[:-1]):
        z = (h @ W.T + b).astype(np.float32)
        r = np.abs(z) / np.abs(z).max()
        found.extend((len(calls), li, int(i), int(j), float(r[i, j])) for i, j in zip(*np.nonzero(r <= rel)))
        h = np.maximum(z, 0)
    return real(layers, x, masks, activation=activation)
  out = []
  for k in range(1, steps + 1):
    calls.clear(); found.clear()
    onets.mlp_forward = recording
    try:
      osac.sac_update(st, c['batches'][k - 1], c['eps_next'][k - 1], c['eps_cur'][k - 1], discount=c['discount'], entropy_target=c['entropy_target'], polyak_factor=c['polyak'], lr=c['lr'],
                      weight_decay=c['weight_decay'])
    finally:
      onets.mlp_forward = real
    out += [(k,) + f for f in found]
  return out


def test_the_rejected_routed_base_is_a_relu_kink():
  """Base 2900 of the routed family at (hidden 256, B 17): exactly one ReLU pre-activation of the back-propagated passes lies within 1e-6 of its layer's scale of zero -
  update 2, the stepped critic 1 on (s, a~) (forward 7), second layer, row 16, unit 202, at 3.9e-8 - and what it back-propagates is that sample's dQ/da, i.e. the
  actor gradient the case missed. The base in use has none. No kernel runs here: the oracle alone."""
  def case(base):
    c = gi.sac_case(base + 17 + 256, NARROW, 256, 17, 2)
    G._free_last_column(NARROW, c['B'], *c['batches'])
    return c
  kinks = _relu_kinks(case(2900))
  assert [k[:5] for k in kinks] == [(2, 7, 1, 16, 202)] and kinks[0][5] < 1e-7, kinks
  assert _relu_kinks(case(SEEDS['routed'])) == []


def test_fused_shape_bc_and_pretrain_plan_at_a_ragged_batch():
  """`behavioural_cloning_update` with a fused-shape actor at B = 100 against osac.bc_update (il_bc_step refuses the batch like il_sac does), and `PretrainPlan('BC')` at that
  batch against the per-function steps on the same batches: the same bits, as at every other batch (tests/test_pretrain_plan_gpu.py)."""
  c = gi.sac_case(SEEDS['routed'] + 1, NARROW, 128, 100, 2)
  _actor_calls('fused shape, ragged batch', c, NARROW, (1, 100), False)
  S, A = NARROW
  tr = gi.transitions(np.random.RandomState(SEEDS['routed'] + 2), 230, S, A, weighted=True)
  t = {k: torch.from_numpy(tr[k]) for k in ('states', 'actions', 'rewards', 'next_states', 'terminals', 'timeouts', 'weights')}
  t['num_trajectories'] = 3
  mem = P.il.ReplayMemory(230, S, A, False, transitions=t, device=P.DEV)
  actors = [P.make_sac(c)[0] for _ in range(2)]
  opts = [P.il.AdamW(a, lr=2.5e-4, weight_decay=0.01) for a in actors]
  plan = P.il.PretrainPlan('BC', actors[0], opts[0], mem, 100, torch.Generator().manual_seed(5), chunk_batches=2)   # two batches per epoch (30 rows dropped), a table of 4: 5 iterations wrap it
  assert plan.general and plan._loss.numel() == 1
  plan.run(5)
  g, count = torch.Generator().manual_seed(5), 5
  while count > 0:   # train.py::expert_batches + the per-function update
    order = torch.randperm(230, generator=g).to(torch.int32)
    for lo in range(0, min(230 - 100 + 1, count * 100), 100):
      loss = P.il.behavioural_cloning_update(actors[1], P.il_memory.batch_views(mem.gather(order[lo:lo + 100]), S, A, False), opts[1])
      count -= 1
  torch.cuda.synchronize()
  for name, x, y in (('parameters', actors[0].flat, actors[1].flat), ('exp_avg', opts[0].exp_avg, opts[1].exp_avg), ('exp_avg_sq', opts[0].exp_avg_sq, opts[1].exp_avg_sq)):
    np.testing.assert_array_equal(P.N(x), P.N(y), err_msg=name)
  np.testing.assert_array_equal(P.N(plan.loss).reshape(-1), P.N(loss).reshape(-1))
  assert int(opts[0].step_count[0]) == 5 and not np.array_equal(P.N(actors[0].flat), c['actor'])


test_fused_shape_bc_and_pretrain_plan_at_a_ragged_batch.streams = True


def test_fused_entry_points_still_refuse_a_ragged_batch():
  """The library's fused entry points keep their refusal (the captured plans, the population sweep and the data-parallel runner reach them directly): il_sac_update and
  il_bc_step at B = 100, their own messages, parameters untouched."""
  c = gi.sac_case(SEEDS['routed'] + 3, NARROW, 128, 100, 1)
  actor, critic, target, log_alpha, ao, co, to = P.make_sac(c)
  before = P.N(actor.flat), P.N(critic.flat)
  b = P.il_training.batch_desc(P.tbatch(c['batches'][0]))
  d = P.il_training.sac_descriptor(actor, critic, log_alpha, target, 100, ao, co, to, 0.97, -1.5, 0.99, general=False)
  logp, q = torch.empty(100, device=P.DEV), torch.empty(100, device=P.DEV)
  with pytest.raises(RuntimeError, match='il_sac: batch=100 must be a positive multiple of 16'):
    P._lib.check(P._lib.lib().il_sac_update(C.byref(d), C.byref(b), None, None, P._lib.ptr(logp), P._lib.ptr(q), 0, P._lib.stream_ptr()))
  ws = torch.zeros(int(P._lib.lib().il_sac_workspace_floats(c['S'], c['A'], 128, 112)), device=P.DEV)
  od = ao.desc()
  with pytest.raises(RuntimeError, match='il_bc_step: batch=100 must be a positive multiple of 16'):
    P._lib.check(P._lib.lib().il_bc_step(P._lib.ptr(actor.flat), P._lib.ptr(ao.grad), C.byref(od), c['S'], c['A'], 128, C.byref(b), P._lib.ptr(ws), ws.numel(), P._lib.ptr(logp), 0, P._lib.stream_ptr()))
  np.testing.assert_array_equal(P.N(actor.flat), before[0]); np.testing.assert_array_equal(P.N(critic.flat), before[1])


# ------------------------------------------------------------------------------------------------ Adam, Polyak
@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 257, 1025, 65537])
def test_adam_and_polyak_on_unaligned_views(n):
  """il_adam_step and il_polyak (test_adam_and_polyak_kernels' bounds) on views whose base is 0, 1, 2 or 3 floats off a 16-byte boundary, independently for the parameter
  (Polyak: the target) and the gradient (Polyak: the source): the vector body, its scalar head and tail. 32 guard floats on each side of every view stay what they were."""
  rs = np.random.RandomState(n)
  G_ = 32
  p0, gr = rs.standard_normal(n).astype(np.float32), (rs.standard_normal(n) * rs.uniform(1e-6, 1, n)).astype(np.float32)
  tgt0 = rs.standard_normal(n).astype(np.float32)

  def view(values, off, fill):
    buf = np.full(G_ + off + n + G_, fill, np.float32); buf[G_ + off:G_ + off + n] = values
    t = P.T(buf)
    return t, t[G_ + off:G_ + off + n], buf

  def guards_intact(t, off, fill, what):
    got = P.N(t)
    assert (got[:G_ + off] == fill).all() and (got[G_ + off + n:] == fill).all(), f'{what}: guard floats overwritten (offset {off})'
  for po in range(4):
    for go in range(4):
      p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
      pbuf, pt, _ = view(p, po, 7.5)
      opt = P.il.AdamW(pt, lr=3e-4, weight_decay=0.1)
      for t in range(1, 3):
        gbuf, gt, _ = view(gr * t, go, -3.25)
        opt.step(gt)
        onets.adam_step(p, gr * t, m, v, t, 3e-4, 0.1)
        np.testing.assert_allclose(P.N(pt), p, rtol=2e-7, atol=1e-9); np.testing.assert_allclose(P.N(opt.exp_avg_sq), v, rtol=2e-7, atol=0)
        guards_intact(gbuf, go, -3.25, 'gradient'); np.testing.assert_array_equal(P.N(gt), gr * t)
      guards_intact(pbuf, po, 7.5, 'parameters')
      tgt = tgt0.copy()
      tbuf, tt, _ = view(tgt, go, 11.0)   # target at the gradient's offset, source = the parameters at theirs
      P._lib.check(P._lib.lib().il_polyak(P._lib.ptr(tt), P._lib.ptr(pt), n, 0.995, P._lib.stream_ptr()))
      onets.polyak(tgt, p, 0.995)
      np.testing.assert_allclose(P.N(tt), tgt, rtol=2e-7, atol=1e-9)
      guards_intact(tbuf, go, 11.0, 'target'); guards_intact(pbuf, po, 7.5, 'polyak source')


# ------------------------------------------------------------------------------------------------ GMMIL, PWIL
GMMIL_EDGE_SHAPES = ((1, 65, 14, 11), (2, 3, 14, 11), (15, 17, 23, 17), (17, 15, 132, 124), (63, 257, 14, 11), (257, 63, 3, 2), (129, 127, 120, 112), (1, 2, 1, 1), (33, 31, 128, 120), (16, 16, 16, 8))


@pytest.mark.parametrize('dims', GMMIL_EDGE_SHAPES, ids=lambda d: 'x'.join(str(x) for x in d))
def test_gmmil_at_edge_sizes(dims):
  """il_gmmil_reward / il_gmmil_sqdist against float64, the body and bound of test_gmmil_direct_form_matches_float64_outside_the_mfma_range (three calls each): a single
  policy row, two and three rows, sets on both sides of 16, 64, 128 and 256 rows, D = 1 .. 132. No shape has a single EXPERT row (module docstring)."""
  assert dims[1] >= 2
  P.test_gmmil_direct_form_matches_float64_outside_the_mfma_range(dims)


@pytest.mark.parametrize('Nn,Th,name', [(255, 5, 'step'), (255, 1, 'one_workgroup'), (256, 5, 'step'), (256, 1, 'one_workgroup'), (257, 5, 'step'), (257, 1, 'one_workgroup'), (513, 5, 'step'),
                                        (513, 2, 'one_workgroup')])
def test_pwil_at_edge_atom_counts(Nn, Th, name, dims=NARROW):
  """The body of test_pwil_at_edge_widths at D = 14 with 255, 256, 257 and 513 atoms (one chunk of 256 atoms short by one, full, one atom into the second, one into the
  third), each at a horizon that takes the one-launch k_pwil_step (m = ceil(N / T) + 2 <= 256) and at one that takes the one-workgroup k_pwil_reward (m > 256)."""
  G.test_pwil_at_edge_widths(dims, name, Nn, Th)


def test_pwil_at_one_by_one():
  test_pwil_at_edge_atom_counts(257, 5, 'step', dims=ONE)


# ------------------------------------------------------------------------------------------------ the first width past each limit
def _disc_cfg(hidden, depth=1, activation='relu', shaping=False):
  return P.Cfg(state_only=False, spectral_norm=True, loss_function='BCE', grad_penalty=0.5, mixup_alpha=1, entropy_bonus=0.01, pos_class_prior=0.7, nonnegative_margin=float('inf'),
               discriminator=P.Cfg(hidden_size=hidden, depth=depth, activation=activation, reward_shaping=shaping, subtract_log_policy=False, reward_function='AIRL'))


def test_shaped_gail_refuses_hidden_257():
  with pytest.raises(NotImplementedError, match='hidden_size <= 256'):
    P.il.GAILDiscriminator(11, 3, _disc_cfg(257, shaping=True), 0.97, device=P.DEV)
  # and the library itself, for a caller that gets past the Python layer
  g = gi.gail_shaped_case(1, NARROW, 256, 16, 1, True)
  d = P.il.GAILDiscriminator(11, 3, _disc_cfg(256, shaping=True), 0.97, device=P.DEV)
  before = P.N(d.flat)
  d.hidden = 257
  with pytest.raises(RuntimeError, match=r'il_disc_shaped: dims out of range \(state=11, input=14, hidden=257; hidden <= 256\)'):
    P.il.adversarial_imitation_update(None, d, P.tbatch(g['policy'][0]), P.tbatch(g['expert'][0]), P.il.AdamW(d, lr=1e-3, weight_decay=0.0), _disc_cfg(256, shaping=True), eps_gp=P.T(g['eps'][0]))
  np.testing.assert_array_equal(P.N(d.flat), before)


@pytest.mark.parametrize('hidden', [3, 258])
def test_red_and_dril_refuse_an_odd_width_and_258(hidden):
  with pytest.raises(NotImplementedError, match=rf'REDDiscriminator: input 14 \(<= 128\) / hidden {hidden} \(even, <= 256\) outside the kernel limits'):
    P.il.REDDiscriminator(11, 3, P.Cfg(state_only=False, reward_bandwidth_scale=None, discriminator=P.Cfg(hidden_size=hidden, depth=1, activation='relu', input_dropout=0, dropout=0)), device=P.DEV)
  with pytest.raises(NotImplementedError, match=rf'DRIL policy: state 11 \(<= 128\), action 3 \(<= 8\), hidden {hidden} \(even, <= 256\) outside the kernel limits'):
    P.il.SoftActor(11, 3, P.Cfg(hidden_size=hidden, depth=1, activation='tanh', input_dropout=0.1, dropout=0.1), device=P.DEV)
  # the library's own check, under a module of the nearest legal width
  c = gi.red_case(1, NARROW, 4, 16, 1)
  d = P.il.REDDiscriminator(11, 3, P.Cfg(state_only=False, reward_bandwidth_scale=None, discriminator=P.Cfg(hidden_size=4, depth=1, activation='relu', input_dropout=0, dropout=0)), device=P.DEV)
  before = P.N(d.flat)
  d.hidden = hidden
  with pytest.raises(RuntimeError, match=rf'il_red: unsupported dims \(input=14, hidden={hidden}\)'):
    P.il.target_estimation_update(d, P.tbatch(c['batches'][0]), P.il.AdamW(d, lr=1e-3, weight_decay=0.0))
  np.testing.assert_array_equal(P.N(d.flat), before)


def test_deep_discriminators_refuse_hidden_129_and_1():
  for shaping in (False, True):
    with pytest.raises(NotImplementedError, match='hidden_size <= 128'):
      P.il.GAILDiscriminator(11, 3, _disc_cfg(129, 2, 'tanh', shaping), 0.97, device=P.DEV)
  with pytest.raises(NotImplementedError, match='hidden_size=1,'):
    P.il.GAILDiscriminator(11, 3, _disc_cfg(1, 2, 'tanh', True), 0.97, device=P.DEV)
  # hidden 1 without shaping passes the Python layer: the library refuses it at the first update, parameters untouched
  c = gi.gail_deep_case(seed=1, env=NARROW, hidden=1, batch=16, steps=1, depth=2, activation='tanh')
  d = P.il.GAILDiscriminator(11, 3, _disc_cfg(1, 2, 'tanh'), 0.97, device=P.DEV)
  before = P.N(d.flat)
  with pytest.raises(RuntimeError, match=r'il_disc_deep: unsupported dims \(input=14 <= 128, hidden=1 <= 128\)'):
    P.il.adversarial_imitation_update(None, d, P.tbatch(c['policy'][0]), P.tbatch(c['expert'][0]), P.il.AdamW(d, lr=1e-3, weight_decay=0.1), _disc_cfg(1, 2, 'tanh'), eps_gp=P.T(c['eps'][0]))
  np.testing.assert_array_equal(P.N(d.flat), before)


def test_gail_discriminator_refuses_a_width_that_is_not_a_multiple_of_16():
  g = gi.gail_case(1, env=NARROW, hidden=24, batch=16, steps=1)
  d = P.il.GAILDiscriminator(11, 3, _disc_cfg(24), 0.97, device=P.DEV)
  before = P.N(d.flat)
  with pytest.raises(RuntimeError, match=r'il_disc: dims out of range \(D=14, hidden=24: hidden must be a multiple of 16\)'):
    P.il.adversarial_imitation_update(None, d, P.tbatch(g['policy'][0]), P.tbatch(g['expert'][0]), P.il.AdamW(d, lr=1e-4, weight_decay=1.0), _disc_cfg(24), eps_gp=P.T(g['eps'][0]))
  np.testing.assert_array_equal(P.N(d.flat), before)
  with pytest.raises(RuntimeError, match='hidden must be a multiple of 16'):
    d.predict_reward(P.T(g['policy'][0]['states']), P.T(g['policy'][0]['actions']))
