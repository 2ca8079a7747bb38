"""`-m gpu`: every kernel family against its oracle at the VALUES where the kernels branch. The sibling modules cover the shapes (tests/test_dim_edges_gpu.py: state and
action widths; tests/test_size_edges_gpu.py: batches and hidden widths); every input of theirs is standard normal with fan-in scaled weights, so a raw log-std stays in
(-1, 1), a discriminator logit in (-3, 3), no two distances are equal and no weight is 0. Here the inputs are edited (tests/golden/inputs.py actor_head_edges,
logit_edge_rows, zero_weight_rows, pwil_tied_case, gmmil_value_edge_case, ADAM_EDGE_GRADS) and the SAME bodies run, with their bounds unchanged: each body is its sibling in
tests/test_size_edges_gpu.py taking a prepared case or an `edit` hook. Everything device-side is reached through the names of tests/test_gpu_parity.py (`P.il`, `P.T`, ...),
which tests/test_value_edges_emulated.py rebinds to the host emulation of the kernels. Sizes: the smallest at which each kernel still runs all its tiles.

Value branches, where they are, and the case that drives each:
  log-std clamp, forward `expf(fminf(fmaxf(lsr, -20.f), 2.f))`: il_common.hpp:399 (head_sample), sac.hip:994, 2964, 3116, general.hip:233, 285, 594, 617, dril.hip:105
  its gradient mask `(lsr >= -20.f && lsr <= 2.f) ? dsd * sd : 0.f`, inclusive at both ends like torch.clamp:
    sac.hip:1046 (il_sac_update)                       test_fused_sac_update_at_the_actor_head_edges
    sac.hip:2972 (il_bc_step)                          test_actor_calls_and_bc_at_the_actor_head_edges[fused-*]
    general.hip:241 (BC, layer at a time)              test_actor_calls_and_bc_at_the_actor_head_edges[general-H33-*]
    general.hip:290 (SAC, layer at a time)             test_general_sac_update_at_the_actor_head_edges[H33-*]
    general.hip:601 (BC, tile engine)                  test_actor_calls_and_bc_at_the_actor_head_edges[general-H48-*]
    general.hip:621 (SAC, tile engine)                 test_general_sac_update_at_the_actor_head_edges[H48-*]
    dril.hip:114 (il_dril_bc_step)                     test_dril_at_the_actor_head_edges
  saturated tanh-Gaussian head (il_common.hpp:398 head_sample and its copies, sac.hip:2967 / 3120, general.hip:237 / 598, dril.hip:109): a = tanhf(x) == +-1 for |x| > 9,
    1 - a a == 0, ladj through the z > 20 branch of softplus_f (il_common.hpp:395; at x = -50 the only finite one: expf(100) overflows), given actions clamped to
    +-(1 - 1e-6) in front of atanhf: all the actor-head cases (means of +12, -12 and -50; given actions of +-1, 0.9999999, 0, -0.0)
  saturated discriminator logits: sigmoid_f (expf overflows below -88, D == 1.0 above 16.7), the reward heads -log1pf(-D + 1e-6f) / logf(D + 1e-6f) - log1pf(-D + 1e-6f) /
    expf(h) * -h at disc_reward.hpp:176 (k_gail_reward and the inline relabel), gail_deep.hip:201, gail_shaped.hip:383, gail_shaped_deep.hip:385, and softplus_f / sigmoid_f
    in the BCE, PUGAIL (gail.hip:366, gail_shaped.hip:215, gail_deep.hip:98, gail_shaped_deep.hip:236: the margin's batch sums) and Mixup gradients: test_*_at_saturated_logits
  PWIL ties: argmin_combine (pwil.hip:21), pw_key (pwil.hip:90) and the ranks of k_pwil_select, the merge, k_pwil_step and k_pwil_couple - "the lowest index wins", five
    times restated: test_pwil_with_tied_atoms (three launch paths), test_pwil_relabel_rows_with_tied_atoms. `il_pwil_act_reward` (the acting-coupled launch) is left out:
    tests/test_pwil_acting_gpu.py builds its atoms, its actor and its episode script inside one body keyed by name, and runs k_pwil_couple, which the relabel case covers
  weights of exactly 0, every terminal 1 / 0, every row absorbing: test_*_with_zero_weights, test_*_with_uniform_flags
  GMMIL: fmaxf(ssq, 0) of the centred Gram form (gmmil.hip, k_gmmil_mfma `finish`) on duplicate rows, v_exp_f32's denormal flush where exp(-gamma d) underflows:
    test_gmmil_with_duplicate_rows_and_zero_weights
  Adam: (1 - beta2) g g on exact zeros, squares that are denormal, underflow or come near FLT_MAX (il_common.hpp:270 adam_update): test_adam_on_edge_gradients

Conditions on the INPUTS, asserted on the oracle's side (EdgeNotMet) so that a change of seeds cannot empty a case without notice:
  (a) every log-std value a case's components were given is met by a (row, component) of the oracle's forward - > 2, < -20, == 2.0 and == -20.0 to the bit (the weight rows of
      those two units are zero: the output IS the bias) - a sampled action is exactly +-1, and (A > 2) a pre-tanh sample lies below -44.4;
  (b) the oracle's logits of the compared rows hold one > 20 and one < -88, and NONE in (8, 17.5): there log1p(-D + 1e-6) turns one ulp of the sigmoid into up to 6 % of its
      argument, two correct float32 evaluations differ, and the sibling's rtol would measure libm against libm. A condition the inputs are built to meet, not a filter: zero
      rows are left out. The PUGAIL case with a margin of 0.02 also asserts that the oracle's clamp does NOT bind while its sums hold a softplus past expf's overflow;
  (d) the atoms are three copies of each row and agent[1] is an atom; (e) duplicate rows at distance exactly 0, the zero weights, the first bandwidth underflows and the
      second is ~1; (f) Adam's v holds a denormal, an underflow to 0 and a value above 1e36.
Bounds: the siblings', unchanged; FLT_MIN as atol for Adam's v (a float32 denormal in v may be flushed by a device: not an error, and FLT_MIN bounds it exactly - the
MI355X keeps them: all three of p, m, v come out bit-identical to numpy). Where `close`'s atol - relative to the LARGEST element - would hide everything else, the same
bound is applied per group: rewards in three groups of |r| (< 2, < 20, the rest: FAIRL reaches -1.4e7 beside rows of 0.3), Adam's first moment of the BC / DRIL
lower-clamp cases per output unit and per earlier layer (sd = e^-20 puts 1e16 into two output units).

Seeds (SEEDS): one base per family, fixed. Rejected for condition (b), on the oracle alone: gail 2100 (logits of 10.7 and 15.7 .. 16.0), 2101 (lowest logit -69), 2102
(10.9, 16.6), 2103 in use (the PUGAIL clamp does not bind there either); deep 2100 (every logit positive: 0.15 .. 562), 2101 (-3.2 .. 80), 2102 in use. No base was
rejected for a comparison.

Found by this module: k_gmmil_mfma at a bandwidth of 1e4 / median - the centred Gram form leaves ssq = +-1e-6 where duplicate rows are 0 apart, and gamma multiplies it:
similarity, self-similarity and reward off by 1.9, 4.8 and 3.1 x the bound on the emulated kernels (the direct forms: 0.01). Such a pair now takes its ssq from the
operands (gmmil.hip, in front of `finish`); with it 0.017 (emulated) / 0.016 (MI355X).

Broken on purpose once, in a scratch copy, on the emulated kernels (each line: the cases that then fail):
  mask sac.hip:1046, `<= 2.f` -> `<` and `>= -20.f` -> `>`: fused_sac_update_at_the_actor_head_edges[64], [128] (each)
  mask sac.hip:2972: `<`: actor_calls_and_bc_at_the_actor_head_edges[fused-H64-*-upper], [-lower], [fused-H128-*-upper], [-lower]; `>`: the two [-lower] cases
  mask general.hip:241: `<`: actor_calls_and_bc...[general-H33-tanh-S11A3-upper], [-lower]; `>`: [general-H33-tanh-S11A3-lower]
  mask general.hip:290: `<`: general_sac_update_at_the_actor_head_edges[H33-d2-tanh-S11A3-from1], [H33-d2-tanh-S1A1]; `>`: [H33-d2-tanh-S11A3-from1]
  mask general.hip:601: `<`: actor_calls_and_bc...[general-H48-relu-S11A3-upper], [-lower]; `>`: [general-H48-relu-S11A3-lower]
  mask general.hip:621: `<` and `>`: general_sac_update_at_the_actor_head_edges[H48-d2-relu-S11A3-from1] (each)
  mask dril.hip:114: `<`: dril_at_the_actor_head_edges[upper], [lower]; `>`: [lower]
    (general.hip:241 / 290 `>` and 621 `<` passed a first version in which each hidden width saw only half of the cycle: hence the `from1` / `from4` pairs per engine)
  softplus_f without its `z > 20` branch: every actor-head case with A > 2 (non-finite log pi at x = -50: 16 cases) and gail_discriminator_at_saturated_logits[PUGAIL-margin-*]
    (a NaN sum makes the clamp bind). With means of +-12 alone it passed everything: log1pf(expf(24)) IS 24.0f, the branch only matters past expf's overflow - hence the
    mean of -50 and the margin case's condition that the oracle's clamp does not bind
  argmin_combine preferring the higher index (pwil.hip:22 `oi > imin`): pwil_with_tied_atoms[600-2-one_workgroup] (k_pwil_reward is its only user)
  pw_key with the index dropped (pwil.hip:90): pwil_with_tied_atoms[4500-18-two_launches_serial_merge] (other atoms survive than in the oracle, step 0); [600-5-step] and
    pwil_relabel_rows_with_tied_atoms do not END on the emulated kernels (equal keys, equal ranks; cut off after 120 s, 4 s unbroken); [600-2-one_workgroup] has no keys
  `1e-6f` removed from a reward head: disc_reward.hpp:176 logf(D): gail_discriminator_at_saturated_logits[*-AIRL], [*-FAIRL] (8 cases) and inline_relabel_heads_at_saturated_logits
    [AIRL], [FAIRL] (non-finite); gail_deep.hip:201 -log1pf(-D): gail_deep_at_saturated_logits[PUGAIL-GAIL]; gail_shaped.hip:383 and gail_shaped_deep.hip:385 (one term
    each): their [BCE-AIRL] and [Mixup-FAIRL] cases

Largest measured deviation over its bound per family: RECORDS below. The emulated module takes 30 s here."""
import contextlib
import json
import os
import atexit

import numpy as np
import pytest
import torch

import inputs as gi
import test_dim_edges_gpu as G
import test_gpu_parity as P
import test_size_edges_gpu as Z
from oracle import gail as ogail
from oracle import nets as onets
from oracle import pwil as opwil

pytestmark = pytest.mark.gpu

NARROW, WIDER, ONE = Z.NARROW, Z.WIDER, Z.ONE
ABSORBING = (18, 6)   # (17, 6) with its absorbing bit (halfcheetah): the widths of `imitation.absorbing=false` have no absorbing rows to make
# ONE base per family, fixed; every case runs at base + its sizes, nothing is drawn again or filtered (module docstring: the bases that were tried)
SEEDS = dict(fused=3100, general=3200, actor=3300, bc=3400, dril=3500, gail=2103, shaped=3600, deep=2102, shaped_deep=3800, weights=3900, flags=4000, pwil=31)
FLT_MIN = float(np.finfo(np.float32).tiny)

# family -> largest measured deviation over its bound, (emulated kernels, MI355X): the whole module, 64 of 64 cases on both. Adam: p, m and v bit-identical to numpy on both
# (the MI355X keeps float32 denormals in v). GMMIL: the largest of the three errors of gmmil_against_float64 over its bound, AFTER the change to k_gmmil_mfma the module led
# to (before it, emulated: 4.8). PWIL asserts equality and its sibling's rtol directly and is not listed. No case is left to the GPU alone, none was not run on it.
RECORDS = {
    'Adam m': (0, 0),
    'Adam p': (0, 0),
    'Adam v': (0, 0),
    'DRIL': (0.0051, 0.0032),
    'DRIL (parameters)': (2.4e-05, 2.4e-05),
    'DRIL, lower clamp (per slab)': (0.01, 0.01),
    'GMMIL': (0.017, 0.016),
    'RED': (0.058, 0.058),
    'RED (parameters)': (2.9e-05, 2.9e-05),
    'fused BC, zero weights': (0.087, 0.094),
    'fused BC, zero weights (parameters)': (0.00011, 0.00011),
    'fused SAC': (0.083, 0.083),
    'fused actor calls, lower clamp': (0.071, 0.071),
    'fused actor calls, lower clamp (parameters)': (3e-05, 3e-05),
    'fused actor calls, lower clamp (per slab)': (0.044, 0.044),
    'fused actor calls, upper clamp': (0.074, 0.074),
    'fused actor calls, upper clamp (parameters)': (5.9e-05, 5.9e-05),
    'gail_deep': (0.036, 0.036),
    'gail_shaped_deep': (0.016, 0.016),
    'general BC, zero weights': (0.072, 0.072),
    'general BC, zero weights (parameters)': (0.00011, 5.7e-05),
    'general SAC': (0.076, 0.076),
    'general SAC (parameters)': (8.2e-05, 8.2e-05),
    'general SAC, uniform flags': (0.095, 0.084),
    'general SAC, uniform flags (parameters)': (0.00019, 0.00019),
    'general SAC, zero weights': (0.13, 0.089),
    'general SAC, zero weights (parameters)': (0.0015, 0.00037),
    'general actor calls, lower clamp': (0.099, 0.099),
    'general actor calls, lower clamp (parameters)': (3e-05, 3e-05),
    'general actor calls, lower clamp (per slab)': (0.013, 0.013),
    'general actor calls, upper clamp': (0.099, 0.099),
    'general actor calls, upper clamp (parameters)': (1.5e-05, 1.5e-05),
    'plain GAIL': (0.042, 0.055),
    'shaped GAIL': (0.034, 0.034),
}

WORST = {}   # this run's figures, written to $IL_VALUE_EDGES_RECORD as JSON when the process ends


@atexit.register
def _write_records():
  if os.environ.get('IL_VALUE_EDGES_RECORD') and WORST:
    with open(os.environ['IL_VALUE_EDGES_RECORD'], 'w') as f: json.dump(WORST, f, indent=1, sort_keys=True)


@contextlib.contextmanager
def _recording():
  """The sibling bodies note their largest deviation over its bound in tests/test_size_edges_gpu.py's WORST, by family: while a case of this module runs, in WORST here."""
  saved, Z.WORST = Z.WORST, WORST
  try: yield
  finally: Z.WORST = saved


class EdgeNotMet(AssertionError):
  """A condition on the INPUTS, checked on the oracle's side: the case no longer holds the values it is about (or holds one it is built to avoid)."""


def _met(cond, what):
  if not cond: raise EdgeNotMet(what)


# ------------------------------------------------------------------------------------------------ (a) the actor head
def _head(c, s, key='actor'):
  out, _ = onets.mlp_forward(onets.unpack(c[key], onets.mlp_shapes(c['S'], c['H'], c['depth'], 2 * c['A'])), s, activation=c['activation'])
  mean, ls_raw, _, std = onets.actor_head(out, c['A'])
  return mean, ls_raw, std


def _assert_head_edges(values, mean, ls_raw, std, eps=None):
  """On the oracle's side: every edge the components of this case were given is met by at least one (row, component) - and a sampled action is +-1 to the bit."""
  met = {3.0: (ls_raw > 2).any(), -25.0: (ls_raw < -20).any(), 2.0: (ls_raw == np.float32(2)).any(), -20.0: (ls_raw == np.float32(-20)).any(),
         1.9: ((ls_raw > 1.5) & (ls_raw != np.float32(2))).any(), 0.0: ((ls_raw > -1) & (ls_raw < 1)).any()}
  for v in values: _met(met[v], f'no raw log-std at the edge {v} (components: {values})')
  if eps is not None:
    x = mean + eps * std
    _met((np.abs(np.tanh(x)) == 1).any(), 'no sampled action is exactly +-1')
    _met(mean.shape[1] < 3 or (-2 * x > 88.8).any(), 'no pre-tanh sample below -44.4 (softplus(-2 x) past the overflow of expf)')


def _sac_head_case(seed, dims, hidden, batch, steps, shift=0, **kw):
  c = gi.sac_case(seed, dims, hidden, batch, steps, **kw)
  values = gi.actor_head_edges(c, shift=shift)
  G._free_last_column(dims, c['B'], *c['batches'])   # (the body does this again: the same draws)
  for k in range(steps):   # the policy pass on s and the target pass on s' of every update
    _assert_head_edges(values, *_head(c, c['batches'][k]['states']), c['eps_cur'][k]); _assert_head_edges(values, *_head(c, c['batches'][k]['next_states']), c['eps_next'][k])
  return c, values


@pytest.mark.parametrize('hidden', [64, 128])
def test_fused_sac_update_at_the_actor_head_edges(hidden):
  """il_sac_update (csrc/sac.hip), one update at batch 48, (17, 6): all six log-std edges, means of +-12."""
  with _recording():
    c, values = _sac_head_case(SEEDS['fused'] + hidden, WIDER, hidden, 48, 1)
    assert set(values) == set(gi.VALUE_EDGE_LOG_STD)
    Z._fused_sac_body(c, WIDER, 48, hidden)


# A = 3 holds three of the six values: each engine of general.hip (layer at a time at hidden 33, tiles at hidden 48) runs the cycle from its second value (-25, 2.0, -20.0)
# and from its fifth (0.0, 1.9, 3.0); (1, 1) holds 2.0 alone, on a component whose mean is +12
GENERAL_HEAD_CASES = [pytest.param(h, act, NARROW, shift, id=f'H{h}-d2-{act}-S11A3-from{shift}') for h, act in ((33, 'tanh'), (48, 'relu')) for shift in (1, 4)] + [pytest.param(33, 'tanh', ONE, 2, id='H33-d2-tanh-S1A1')]


def test_each_general_engine_holds_every_log_std_edge():
  """No kernel runs here: the two (11, 3) cases of each hidden width hold the six values between them."""
  for h in (33, 48):
    held = set()
    for hidden, act, dims, shift in (p.values for p in GENERAL_HEAD_CASES):
      if hidden == h and dims == NARROW: held |= set(gi.actor_head_edges(gi.sac_case(1, dims, hidden, 16, 1, depth=2, activation=act), shift=shift))
    assert held == set(gi.VALUE_EDGE_LOG_STD), (h, held)


@pytest.mark.parametrize('hidden,activation,dims,shift', GENERAL_HEAD_CASES)
def test_general_sac_update_at_the_actor_head_edges(hidden, activation, dims, shift):
  """il_sac_update_general (csrc/general.hip: the layer-at-a-time kernels at hidden 33, the tile engine at hidden 48), two updates at batch 17."""
  with _recording():
    c, _ = _sac_head_case(SEEDS['general'] + hidden + dims[0] + shift, dims, hidden, 17, 2, shift=shift, depth=2, activation=activation)
    actor, critic = Z._sac_updates('general SAC', c, dims)
    assert actor.general or critic.general


def _given_action_edges(b):
  """Given actions of exactly +1 and -1 (clamped to +-(1 - 1e-6) before atanhf), 0.9999999 (above the clamp), 0 and -0.0."""
  a = b['actions']
  a[0] = 1; a[1 % len(a)] = -1
  if len(a) > 2: a[2, 0] = np.float32(0.9999999)
  if len(a) > 3: a[3] = 0; a[3, -1] = -0.0


def _slabs(S, H, depth, A):
  """(name, slice) per slab of a flat actor vector: every earlier layer whole, the last layer per output unit (its weight row, then its bias)."""
  out, o = [], 0
  for l, ((rows, cols), _) in enumerate(onets.mlp_shapes(S, H, depth, 2 * A)):
    n = rows * cols + rows
    if l < depth: out.append((f'layer {l}', slice(o, o + n)))
    else: out += [(f'output unit {u}', np.r_[o + u * cols:o + (u + 1) * cols, o + rows * cols + u]) for u in range(rows)]
    o += n
  return out


def _slab_check(family, c, atol_scale):
  """Adam's first moment (0.1 x the gradient after the first step) per slab at the sibling's bound for the whole vector: with sd = e^-20 the gradients of two output
  units reach 1e16, and `close`'s atol - relative to the largest element - would say nothing about the other slabs."""
  def after_step(k, got, want):
    for name, sl in _slabs(c['S'], c['H'], c['depth'], c['A']):
      Z.close(family + ' (per slab)', got[sl], want[sl], f'm {k}, {name}', atol_scale=atol_scale * k)
  return after_step


ACTOR_CALL_CASES = [pytest.param(h, act, general, dims, clamp, id=f'{"general" if general else "fused"}-H{h}-{act}-S{dims[0]}A{dims[1]}-{clamp}')
                    for h, act, general, dims in ((64, 'relu', False, WIDER), (128, 'relu', False, WIDER), (33, 'tanh', True, NARROW), (48, 'relu', True, NARROW)) for clamp in ('upper', 'lower')]


@pytest.mark.parametrize('hidden,activation,general,dims,clamp', ACTOR_CALL_CASES)
def test_actor_calls_and_bc_at_the_actor_head_edges(hidden, activation, general, dims, clamp):
  """il_actor_act / il_actor_log_prob / il_bc_step and their `_general` forms: the sample with fed noise, its log pi, the greedy action, log pi of given actions (+-1,
  0.9999999 and 0 among them) and two BC steps. `upper`: VALUE_EDGE_LOG_STD_UPPER. `lower`: all six values - log pi of given actions is then -1e17 in every row and the
  gradients of two output units 1e16, so Adam's first moment is also compared slab by slab."""
  with _recording():
    batch = 17 if general else 48
    c = gi.sac_case(SEEDS['actor'] + hidden, dims, hidden, batch, 2, depth=2, activation=activation)
    shift = 1 if general and clamp == 'lower' else 0   # A = 3: upper 3.0, 2.0, 0.0; lower -25, 2.0, -20.0
    values = gi.actor_head_edges(c, upper_only=clamp == 'upper', shift=shift)
    G._free_last_column(dims, c['B'] + 1, *c['batches'])
    for b in c['batches']: _given_action_edges(b)
    _assert_head_edges(values, *_head(c, c['batches'][0]['states']), c['eps_cur'][0])
    family = ('general' if general else 'fused') + f' actor calls, {clamp} clamp'
    Z._actor_calls(family, c, dims, (1, 2, 3, 17) if general else (1, 3, 17, 33), general, after_step=_slab_check(family, c, 1e-5) if clamp == 'lower' else None)


@pytest.mark.parametrize('clamp', ['upper', 'lower'])
def test_dril_at_the_actor_head_edges(clamp):
  """il_dril_bc_step and il_dril_uncertainty (csrc/dril.hip) at batch 33, hidden 30, (11, 3): two updates with given dropout masks and the Monte-Carlo uncertainty.
  A = 3 holds three values: `upper` 3.0, 2.0, 0.0; `lower` starts the cycle at its second value: -25, 2.0, -20.0."""
  with _recording():
    held = []

    def edit(c):
      held.extend(gi.actor_head_edges(c, upper_only=clamp == 'upper', shift=0 if clamp == 'upper' else 1, key='params'))
      for b in c['batches']: _given_action_edges(b)
      keep = c['m0'][0] * np.float32(1 / 0.9)   # the first update's forward as oracle/dril.py runs it (input dropout, then hidden dropout in front of the tanh)
      layers = onets.unpack(c['params'], onets.mlp_shapes(c['S'], c['H'], 1, 2 * c['A']))
      h = np.tanh(((c['batches'][0]['states'] * keep) @ layers[0][0].T + layers[0][1]) * (c['m1'][0] * np.float32(1 / 0.9))).astype(np.float32)
      _assert_head_edges(held, *onets.actor_head(h @ layers[1][0].T + layers[1][1], c['A'])[:2], np.float32(1))
    c_dims = dict(S=NARROW[0], A=NARROW[1], H=30, depth=1)
    Z._dril_body(NARROW, 33, 30, edit=edit, after_step=_slab_check('DRIL, lower clamp', c_dims, 1e-5) if clamp == 'lower' else None)
    assert held


# ------------------------------------------------------------------------------------------------ (b) discriminator logits
REWARD_GROUPS = ((0.0, 2.0), (2.0, 20.0), (20.0, float('inf')))   # |r|: the unsaturated rows, the saturated AIRL / GAIL rows (up to 13.8), FAIRL's exp(h) * -h (up to 1.4e7)


def _rows_close(family, got, want, name, logits, rtol, atol_scale):
  """The sibling's bound for the reward, applied per group of rows of like magnitude (a FAIRL reward of -1.4e7 beside rows of 0.3 would hide them in `close`'s atol), after
  the conditions on the oracle's logits of the compared rows: one above 20 (D == 1.0 in float32 from 16.7), one below -88 (expf(-z) overflows), none in (8, 17.5), where
  log1p(-D + 1e-6) turns one ulp of the sigmoid into up to 6 % of its argument and two correct float32 evaluations differ. Zero rows are left out."""
  z = np.asarray(logits, np.float64)
  _met((z > 20).any() and (z < -88).any(), f'{name}: the oracle\'s logits run from {z.min():.4g} to {z.max():.4g}, not past 20 and -88')
  _met(not ((z > 8) & (z < 17.5)).any(), f'{name}: oracle logits in (8, 17.5): {z[(z > 8) & (z < 17.5)]}')
  mag = np.abs(np.asarray(want, np.float64))
  assert np.isfinite(np.asarray(got)).all() and np.isfinite(mag).all()
  for lo, hi in REWARD_GROUPS:
    rows = (mag >= lo) & (mag < hi)
    if rows.any(): Z.close(family, np.asarray(got)[rows], np.asarray(want)[rows], f'{name}, rows with {lo:g} <= |r| < {hi:g}', rtol=rtol, atol_scale=atol_scale)


def _logit_edit(c):
  gi.logit_edge_rows(c['policy'][0]); gi.logit_edge_rows(c['expert'][0])


HEADS = ('AIRL', 'GAIL', 'FAIRL')


@pytest.mark.parametrize('reward_function', HEADS)
@pytest.mark.parametrize('loss,margin', Z.GAIL_LOSSES, ids=['BCE', 'PUGAIL', 'PUGAIL-margin', 'Mixup'])
def test_gail_discriminator_at_saturated_logits(loss, margin, reward_function):
  """il_gail_disc_step / il_gail_reward (csrc/gail.hip, disc_reward.hpp) at batch 33, hidden 48, (17, 6)."""
  with _recording():
    held, seen, real = [], [], onets.softplus

    def edit(g):
      _logit_edit(g); held.append(g)

    def recording(z):
      seen.append((np.array(z), real(z)))
      return seen[-1][1]
    onets.softplus = recording   # (the oracle's PUGAIL margin decision: pr mean(we softplus(z_e)) - mean(wp softplus(z_p)) >= -margin, expert first)
    try:
      Z._gail_body(WIDER, 33, 48, loss, margin, SEEDS['gail'], edit=edit, reward_function=reward_function, reward_close=_rows_close, state_only_values=(False,))
    finally:
      onets.softplus = real
    if margin != float('inf'):
      (ze, se), (zp, sp) = seen[:2]
      V = np.float32(0.7) * np.mean(held[0]['expert'][0]['weights'] * se, dtype=np.float32) - np.mean(held[0]['policy'][0]['weights'] * sp, dtype=np.float32)
      _met(max(ze.max(), zp.max()) > 88.8 and np.isfinite(V) and V >= -margin, f'PUGAIL margin: the sums hold no softplus past expf\'s overflow, or the clamp binds (V = {V})')


DISC_CASES = [pytest.param(*Z.LOSSES3[i], HEADS[i], id=f'{Z.LOSSES3[i][0]}-{HEADS[i]}') for i in range(3)]


@pytest.mark.parametrize('loss,margin,reward_function', DISC_CASES)
def test_shaped_gail_at_saturated_logits(loss, margin, reward_function):
  """il_gail_shaped_step / il_gail_shaped_reward (csrc/gail_shaped.hip) at batch 33, hidden 17, (17, 6), 30 % terminal rows."""
  with _recording():
    Z._shaped_body(WIDER, 33, 17, loss, margin, SEEDS['shaped'], edit=_logit_edit, reward_function=reward_function, reward_close=_rows_close)


@pytest.mark.parametrize('loss,margin,reward_function', DISC_CASES)
def test_gail_deep_at_saturated_logits(loss, margin, reward_function):
  """csrc/gail_deep.hip at batch 33, hidden 17, depth 2, relu (a tanh network cannot reach these logits), (17, 6). (The sibling body has no finite margin.)"""
  with _recording():
    Z._deep_body(WIDER, 33, 17, 2, 'relu', loss, SEEDS['deep'], edit=_logit_edit, reward_function=reward_function, reward_close=_rows_close)


@pytest.mark.parametrize('loss,margin,reward_function', DISC_CASES)
def test_gail_shaped_deep_at_saturated_logits(loss, margin, reward_function):
  """csrc/gail_shaped_deep.hip at batch 33, hidden 17, depth 2, relu, (17, 6), 30 % terminal rows."""
  with _recording():
    c = gi.gail_shaped_deep_case(seed=SEEDS['shaped_deep'], env=WIDER, hidden=17, batch=33, steps=1, depth=2, activation='relu', spectral_norm=True)
    G._free_last_column(WIDER, 6, c['policy'][0], c['expert'][0])
    _logit_edit(c)
    assert c['policy'][0]['terminals'].sum() >= 5
    Z._shaped_deep_body(c, 17, 2, 'relu', loss, reward_function=reward_function, reward_close=_rows_close)


def _ring_edit(tr, etr):
  """Every block of 11 rows of both rings scaled like the rows 0 .. 10 of a batch: whatever the plan draws holds the scaled rows."""
  for t in (tr, etr):
    n = t['states'].shape[0]
    for lo in range(0, n - 10, 11):
      gi.logit_edge_rows({k: t[k][lo:lo + 11] for k in ('states', 'actions', 'next_states', 'weights')}, zero_weights=())


@pytest.mark.parametrize('reward_function', HEADS)
def test_inline_relabel_heads_at_saturated_logits(reward_function):
  """test_inline_relabel_heads_equal_the_reward_kernel (disc_reward.hpp inside the chained SAC launch against k_gail_reward, bit for bit) on rings that hold the scaled
  rows; the logits of the compared rows from the oracle's forward on the discriminator's parameters."""
  plan, nets = P.test_inline_relabel_heads_equal_the_reward_kernel(reward_function, edit=_ring_edit)
  d = nets[4]
  ods = ogail.DiscState(sum(gi.DIMS['halfcheetah']), 64, True)
  ods.unpack_into(P.N(d.flat)); v = d.views()
  for k in ('u1', 'v1', 'u2', 'v2'): getattr(ods, k)[...] = P.N(v[k])
  t = plan.transitions
  z = ogail.disc_logits(ods, np.concatenate([P.N(t['states']), P.N(t['actions'])], 1))
  _met((z > 20).any() and (z < -88).any(), f'inline relabel: the logits of the relabelled rows run from {z.min():.4g} to {z.max():.4g}')


test_inline_relabel_heads_at_saturated_logits.streams = True


# ------------------------------------------------------------------------------------------------ (c) zero weights, uniform flags
def _zero_batches(c):
  for b in c['batches']: gi.zero_weight_rows(b)
  assert all((b['weights'] == 0).sum() >= 2 for b in c['batches'])


def _all_absorbing(b):
  """Every row an absorbing -> absorbing transition (memory.py:62): zero state and action, the absorbing bit set in s and s'."""
  b['states'][:] = 0; b['states'][:, -1] = 1; b['next_states'][:] = 0; b['next_states'][:, -1] = 1; b['actions'][:] = 0
  b['absorbing'] = np.ones(len(b['states']), np.float32)


def _set_flags(b, flags):
  if flags == 'terminal_1': b['terminals'][:] = 1
  elif flags == 'terminal_0': b['terminals'][:] = 0
  else: _all_absorbing(b)


@pytest.mark.parametrize('hidden', [64, 128])
def test_fused_sac_and_bc_with_zero_weights(hidden):
  with _recording():
    c = gi.sac_case(SEEDS['weights'] + hidden, WIDER, hidden, 48, 2)
    _zero_batches(c)
    assert (c['batches'][0]['weights'][16:32] == 0).all()   # one whole 16-row tile
    Z._fused_sac_body(c, WIDER, 48, hidden)
    Z._actor_calls('fused BC, zero weights', c, WIDER, (1, 17), False)


@pytest.mark.parametrize('hidden,activation', [(33, 'tanh'), (48, 'relu')])
def test_general_sac_and_bc_with_zero_weights(hidden, activation):
  with _recording():
    c = gi.sac_case(SEEDS['weights'] + hidden, NARROW, hidden, 17, 2, depth=2, activation=activation)
    _zero_batches(c)
    Z._sac_updates('general SAC, zero weights', c, NARROW)
    c = gi.sac_case(SEEDS['weights'] + hidden + 1, NARROW, hidden, 17, 2, depth=2, activation=activation)
    _zero_batches(c)
    Z._actor_calls('general BC, zero weights', c, NARROW, (1, 17), True)


def test_gail_red_and_dril_with_zero_weights():
  with _recording():
    def disc_edit(g):
      gi.zero_weight_rows(g['policy'][0]); gi.zero_weight_rows(g['expert'][0])
    for loss, margin in Z.GAIL_LOSSES:
      Z._gail_body(WIDER, 48, 48, loss, margin, SEEDS['weights'], edit=disc_edit)   # (B = 48: a whole 16-row tile of zero weights)
    Z._red_body(NARROW, 33, 30, edit=_zero_batches)
    Z._dril_body(NARROW, 33, 30, edit=_zero_batches)


FLAGS = ('terminal_1', 'terminal_0', 'absorbing')


@pytest.mark.parametrize('flags', FLAGS)
def test_sac_with_uniform_flags(flags):
  """Fused (hidden 64, batch 48) and general (hidden 33, tanh, batch 17) SAC with every terminal 1, every terminal 0, and every row absorbing - at (18, 6) / hopper's
  (12, 3), the widths that have an absorbing bit."""
  with _recording():
    c = gi.sac_case(SEEDS['flags'], ABSORBING, 64, 48, 1)
    for b in c['batches']: _set_flags(b, flags)
    Z._fused_sac_body(c, ABSORBING, 48, 64)
    c = gi.sac_case(SEEDS['flags'] + 1, 'hopper', 33, 17, 2, depth=2, activation='tanh')
    for b in c['batches']: _set_flags(b, flags)
    Z._sac_updates('general SAC, uniform flags', c, (0, 0))


@pytest.mark.parametrize('flags', FLAGS)
def test_shaped_gail_with_uniform_flags(flags):
  with _recording():
    def edit(c):
      _set_flags(c['policy'][0], flags)
      if flags != 'absorbing': _set_flags(c['expert'][0], flags)   # (every row of BOTH batches identical would leave the gradient penalty nothing to mix)
    Z._shaped_body(ABSORBING, 33, 17, 'BCE', float('inf'), SEEDS['flags'] + 2, edit=edit)


# ------------------------------------------------------------------------------------------------ (d) PWIL ties
PWIL_PATHS = [(600, 5, 'step'), (600, 2, 'one_workgroup'), (4500, 18, 'two_launches_serial_merge')]


def _pwil_memory(atoms, S, A, ends=()):
  n, t = atoms.shape[0], torch.from_numpy
  flags = torch.zeros(n)
  for r in ends: flags[r] = 1.0
  return P.il.ReplayMemory(n, S, A, False, transitions=dict(states=t(atoms[:, :S]), actions=t(atoms[:, S:]), rewards=torch.zeros(n), next_states=t(atoms[:, :S]), terminals=flags,
                                                            timeouts=torch.zeros(n), weights=torch.ones(n), num_trajectories=4), device=P.DEV)


@pytest.mark.parametrize('Nn,Th,name', PWIL_PATHS)
def test_pwil_with_tied_atoms(Nn, Th, name):
  """The body of test_pwil_at_edge_widths at D = 14 on pwil_tied_case - every atom three times, an agent point ON an atom, a near tie - plus, after EVERY step, the
  surviving atoms under their original indices and their remaining weights, element by element (oracle/pwil.py `alive`)."""
  S, A = NARROW
  steps = 2 * Th + 3
  atoms, agent = gi.pwil_tied_case(SEEDS['pwil'], Nn, S + A, steps)
  _met(len(np.unique(atoms, axis=0)) == Nn // 3 and (atoms == agent[1]).all(1).sum() == 3, 'the atoms are not three copies of each row / agent[1] is not an atom')
  d = P.il.PWILDiscriminator(S, A, P.Cfg(state_only=False, reward_scale=5, reward_bandwidth_scale=5), _pwil_memory(atoms, S, A), Th)
  m, Gn = int(np.ceil((1 / Th - 1e-6) * Nn)) + 2, -(-Nn // 256)
  assert {'one_workgroup': m > 256, 'two_launches_serial_merge': m <= 256 and Gn * m > 4096}.get(name, Gn * m <= 4096 and m <= 256), (m, Gn)
  o = opwil.PwilOracle(atoms, Th, 5, 5)
  got, want = [], []
  for k in range(steps):
    got.append(float(d.compute_reward(P.T(agent[k:k + 1, :S]), P.T(agent[k:k + 1, S:]))))
    want.append(o.compute_reward(agent[k]))
    w, full = P.N(d.expert_weights), np.full(Nn, -1.0, np.float32)
    full[o.alive] = o.weights
    assert ((w >= 0) == (full >= 0)).all(), f'step {k}: other atoms survive than in the oracle: {np.nonzero((w >= 0) != (full >= 0))[0][:10]}'
    np.testing.assert_array_equal(w[w >= 0], full[full >= 0], err_msg=f'step {k}: remaining weights')
    if k % Th == Th - 1:
      d.reset(); o.reset()
  np.testing.assert_allclose(got, want, rtol=2e-5)
  assert int((d.expert_weights >= 0).sum()) == len(o.weights)


def test_pwil_relabel_rows_with_tied_atoms():
  """il_pwil_relabel_rows (k_pwil_couple, the device-resident expert relabel) on the tied set, (600, 5): every relabelled row IS an atom - distance 0, three times - and
  episodes end every five rows. Bit for bit against the row loop through il_pwil_reward: the reward column and the atom weights; the rewards against the oracle."""
  S, A = NARROW
  Nn, Th, count = 600, 5, 20
  atoms, _ = gi.pwil_tied_case(SEEDS['pwil'], Nn, S + A, 3)
  ends = range(Th - 1, Nn, Th)
  cfg = P.Cfg(state_only=False, reward_scale=5, reward_bandwidth_scale=5)
  mem_loop, mem_dev = _pwil_memory(atoms, S, A, ends), _pwil_memory(atoms, S, A, ends)
  d_loop, d_dev = P.il.PWILDiscriminator(S, A, cfg, mem_loop, Th), P.il.PWILDiscriminator(S, A, cfg, mem_dev, Th)
  o = opwil.PwilOracle(atoms, Th, 5, 5)
  want = []
  for i in range(count - 2):   # (the last episode is left open: the atom weights then differ from 1 / N)
    mem_loop.rewards[i] = d_loop.compute_reward(P.T(atoms[i:i + 1, :S]), P.T(atoms[i:i + 1, S:]))
    want.append(o.compute_reward(atoms[i]))
    if i % Th == Th - 1: d_loop.reset(); o.reset()
  d_dev.relabel_memory(mem_dev, first=0, count=count - 2)
  torch.cuda.synchronize()
  col = 2 * S + A
  np.testing.assert_array_equal(P.N(mem_dev.ring)[:, col], P.N(mem_loop.ring)[:, col])
  np.testing.assert_array_equal(P.N(d_dev.expert_weights), P.N(d_loop.expert_weights))
  full = np.full(Nn, -1.0, np.float32); full[o.alive] = o.weights
  w = P.N(d_dev.expert_weights)
  assert ((w >= 0) == (full >= 0)).all() and (w < 0).any()
  np.testing.assert_array_equal(w[w >= 0], full[full >= 0])
  np.testing.assert_allclose(P.N(mem_dev.ring)[:count - 2, col], want, rtol=2e-5)


test_pwil_relabel_rows_with_tied_atoms.streams = True


# ------------------------------------------------------------------------------------------------ (e) GMMIL
GMMIL_SHAPES = ((65, 63, 23, 17), (33, 31, 132, 124))   # k_gmmil_mfma (the centred Gram form, D <= 128) and k_gmmil_direct (D = 132)


@pytest.mark.parametrize('gamma_scales', [(1.0, 1.0), (1e4, 1e-4)], ids=['median', 'underflow-and-one'])
@pytest.mark.parametrize('dims', GMMIL_SHAPES, ids=lambda d: 'x'.join(str(x) for x in d))
def test_gmmil_with_duplicate_rows_and_zero_weights(dims, gamma_scales):
  """The body and bound of test_gmmil_direct_form_matches_float64_outside_the_mfma_range on gmmil_value_edge_case."""
  c = gi.gmmil_value_edge_case(*dims, gamma_scales=gamma_scales)
  n1 = dims[0]
  _met((c['dxx'][np.arange(n1 // 3), np.arange(n1 // 3) + n1 // 3] == 0).all() and (c['dxe'] == 0).sum() >= dims[1] // 3 and (c['w'] == 0).sum() == 3 and (c['we'] == 0).sum() == 2,
       'no duplicate rows / zero weights')
  if gamma_scales[0] > 1:
    off = c['dxe'] > 0
    _met(np.exp(-c['g1'] * c['dxe'][off]).max() < 1e-45 and np.exp(-c['g2'] * c['dxe']).min() > 0.99, 'the first bandwidth does not underflow / the second is not about 1')
  errs = P.gmmil_against_float64(dims, c)
  WORST['GMMIL'] = max(WORST.get('GMMIL', 0.0), float(max(errs)))


# ------------------------------------------------------------------------------------------------ (f) Adam, Polyak
@pytest.mark.parametrize('weight_decay', [0.0, 0.1])
def test_adam_on_edge_gradients(weight_decay):
  """il_adam_step, three steps on ADAM_EDGE_GRADS (x 1, 2, 3) against oracle/nets.py adam_step: parameters and m at the bound of test_adam_at_a_late_step, v at its rtol
  plus FLT_MIN - a float32 denormal in v may be flushed by the device, which is no error and which FLT_MIN bounds exactly. Everything finite: (1 - beta2) g g is
  evaluated as ((1 - beta2) g) g, like torch's addcmul_, which keeps g = 9e19 in range (8.1e36)."""
  gr = gi.ADAM_EDGE_GRADS
  n = gr.size
  assert n % 4 and (gr == 0).any() and (np.abs(gr) == np.float32(3e19)).any()
  p = np.random.RandomState(n).standard_normal(n).astype(np.float32)
  m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
  pt = P.T(p.copy())
  opt = P.il.AdamW(pt, lr=3e-4, weight_decay=weight_decay)
  for t in range(1, 4):
    g = (gr * np.float32(t)).astype(np.float32)
    opt.step(P.T(g))
    with np.errstate(under='ignore'): onets.adam_step(p, g, m, v, t, 3e-4, weight_decay)
    got = P.N(pt), P.N(opt.exp_avg), P.N(opt.exp_avg_sq)
    assert all(np.isfinite(x).all() for x in got) and all(np.isfinite(x).all() for x in (p, m, v))
    np.testing.assert_allclose(got[0], p, rtol=2e-7, atol=1e-9); np.testing.assert_allclose(got[1], m, rtol=2e-7, atol=1e-9)
    np.testing.assert_allclose(got[2], v, rtol=2e-7, atol=FLT_MIN)
    for name, x, y, atol in (('p', got[0], p, 1e-9), ('m', got[1], m, 1e-9), ('v', got[2], v, FLT_MIN)):
      WORST['Adam ' + name] = max(WORST.get('Adam ' + name, 0.0), float((np.abs(x.astype(np.float64) - y) / (2e-7 * np.abs(y.astype(np.float64)) + atol)).max()))
  _met((v[gr == np.float32(1e-20)] < FLT_MIN).all() and (v[gr == np.float32(1e-20)] > 0).all() and (v[gr == np.float32(1e-30)] == 0).all() and v.max() > 1e36,
       'v holds no denormal / no underflow / nothing near the top of the range')


def test_polyak_on_edge_values():
  """il_polyak on a target that holds +-1e30 and 0 (and a source that holds them at other places): the bound of test_adam_and_polyak_kernels."""
  n = 1027
  rs = np.random.RandomState(n)
  edge = np.array([1e30, -1e30, 0.0, -0.0, 1e-30, 1.0], np.float32)
  tgt, src = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
  tgt[::7] = edge[np.arange(len(tgt[::7])) % 6]; src[3::11] = edge[np.arange(len(src[3::11])) % 6]
  tt, st = P.T(tgt.copy()), P.T(src)
  P._lib.check(P._lib.lib().il_polyak(P._lib.ptr(tt), P._lib.ptr(st), n, 0.995, P._lib.stream_ptr()))
  onets.polyak(tgt, src, 0.995)
  assert np.isfinite(P.N(tt)).all()
  np.testing.assert_allclose(P.N(tt), tgt, rtol=2e-7, atol=1e-9)
