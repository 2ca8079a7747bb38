"""`python train.py -m seed=... algorithm=GAIL imitation.loss_function=Mixup +sweep.gail_mixup_population=true` without a GPU: which Mixup sweeps form one population and
which run job after job, and why. The opt-in is a key of its own: without it a Mixup sweep runs as it always has, whatever `+sweep.schedule` or the other algorithms' keys
say (tests/test_sweep_config_cpu.py pins that the reason contains `Mixup`). And the new entry point is bound, exported and refuses on the host."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imitation_learning_amd import config  # noqa: E402,F401
from test_sweep_gmmil_config_cpu import _cfgs, _groups  # noqa: E402

KEY = '+sweep.gail_mixup_population=true'
MIXUP = ['algorithm=GAIL', 'imitation.loss_function=Mixup']


@pytest.mark.parametrize('argv', [MIXUP, MIXUP + ['imitation.mixup_alpha=1'], MIXUP + ['imitation.mixup_alpha=0.5'], ['algorithm=GAIL', 'optimised_hyperparameters=GAIL_5_trajectories'],
                                  ['algorithm=GAIL', 'optimised_hyperparameters=GAIL_10_trajectories'], MIXUP + ['+acting.schedule=fused'], MIXUP + ['env=halfcheetah', 'imitation.state_only=true']],
                         ids=['default-alpha', 'alpha1', 'alpha0.5', 'GAIL_5', 'GAIL_10', 'fused-acting', 'halfcheetah-state_only'])
@pytest.mark.parametrize('schedule', [None, 'population', 'per_learner'])
def test_mixup_seed_sweeps_form_one_population_under_the_key(argv, schedule):
  import train
  cfgs = _cfgs(['seed=1,2'] + argv + [KEY] + ([f'+sweep.schedule={schedule}'] if schedule else []))
  assert cfgs[0].imitation.loss_function == 'Mixup'
  assert train.gail_mixup_population(cfgs[0]) and train.sweep_fallback_reason(cfgs[0]) is None
  assert train.sweep_groups(cfgs) == [([0, 1], None)]
  assert train.sweep_schedule(cfgs[0]) == (schedule or train.SWEEP_DEFAULT_SCHEDULE)


def test_the_shipped_mixup_configurations():
  """What the two tuned Mixup overlays ask of the launch: batch 1024 with spectral norm and an entropy bonus of 0.24, batch 512 without spectral norm; both at hidden 64,
  depth 1, with a gradient penalty (two calls per update)."""
  got = []
  for n in (5, 10):
    c = _cfgs(['seed=1,2', 'algorithm=GAIL', KEY, f'optimised_hyperparameters=GAIL_{n}_trajectories'])[0]
    d = c.imitation.discriminator
    assert c.imitation.loss_function == 'Mixup' and (int(d.depth), str(d.activation), int(d.hidden_size)) == (1, 'relu', 64) and float(c.imitation.grad_penalty) > 0
    got.append((int(c.training.batch_size), bool(c.imitation.spectral_norm), round(float(c.imitation.entropy_bonus), 2)))
  assert got == [(1024, True, 0.24), (512, False, 0.02)]
  c = _cfgs(['seed=1,2', 'algorithm=GAIL', KEY, 'optimised_hyperparameters=GAIL_25_trajectories'])[0]   # BCE: one population with or without the key
  assert c.imitation.loss_function == 'BCE'


@pytest.mark.parametrize('extra', [[], ['+sweep.schedule=population'], ['+sweep.schedule=per_learner'], ['+sweep.gail_mixup_population=false'], ['+sweep.pwil_population=true'],
                                   ['+sweep.adril_population=true'], ['+sweep.schedule=population', '+sweep.pwil_population=true', '+sweep.adril_population=true']],
                         ids=['no-key', 'schedule-population', 'schedule-per_learner', 'key-false', 'pwil-key', 'adril-key', 'every-other-key'])
@pytest.mark.parametrize('alpha', [[], ['imitation.mixup_alpha=0.5']], ids=['alpha1', 'alpha0.5'])
def test_mixup_population_is_asked_for_with_a_key_of_its_own(extra, alpha):
  """Without `+sweep.gail_mixup_population=true` a Mixup sweep keeps running job after job; the reason keeps its words and says how to ask."""
  runs, _ = _groups(['seed=1,2'] + MIXUP + alpha + extra)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  for _, reason in runs:
    assert 'imitation.loss_function=Mixup has no population discriminator step (BCE and PUGAIL with an infinite margin have)' in reason, reason
    assert KEY in reason and 'il_gail_mixup_step_population' in reason, reason


@pytest.mark.parametrize('argv,word', [
    (['imitation.discriminator.reward_shaping=true'], 'reward shaping / subtract_log_policy run their per-function entry points inside the plan'),
    (['imitation.discriminator.subtract_log_policy=true'], 'reward shaping / subtract_log_policy run their per-function entry points inside the plan'),
    (['imitation.discriminator.depth=2'], 'a depth-2 / tanh discriminator runs its per-function entry points inside the plan'),
    (['imitation.discriminator.activation=tanh'], 'a depth-2 / tanh discriminator runs its per-function entry points inside the plan'),
    (['imitation.mix_expert_data=mixed_batch'], 'imitation.mix_expert_data=mixed_batch edits the batches between the launches'),
    (['imitation.bc_aux_loss=true'], 'imitation.bc_aux_loss adds an actor step per update that the population launches do not have'),
    (['training.batch_size=100'], 'training.batch_size=100 is not a multiple of 16'),
    (['reinforcement.actor.depth=3'], 'an actor / critic shape outside depth 2, ReLU, hidden 64..256 in multiples of 64 has no population launches'),
    (['distributed.world_size=2'], 'distributed.world_size > 1: a population is a single-GPU mode')])
@pytest.mark.parametrize('schedule', [None, 'population'])
def test_with_the_key_a_variant_keeps_its_own_reason(argv, word, schedule):
  """With the key, every other condition of a population still holds, in its present words: the variant's reason wins."""
  runs, _ = _groups(['seed=1,2'] + MIXUP + [KEY] + ([f'+sweep.schedule={schedule}'] if schedule else []) + argv)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  assert all(reason == word for _, reason in runs), runs


def test_the_key_opts_no_other_configuration_in():
  import train
  reason = train.sweep_fallback_reason(_cfgs(['seed=1,2', 'algorithm=GAIL', 'imitation.loss_function=PUGAIL', 'imitation.nonnegative_margin=0.05', KEY])[0])
  assert reason == 'a finite PUGAIL margin needs a value pass ahead of the gradients'
  for alg, word in (('PWIL', '+sweep.pwil_population=true'), ('AdRIL', '+sweep.adril_population=true'), ('BC', 'algorithm=BC has no population launches')):
    reason = train.sweep_fallback_reason(_cfgs(['seed=1,2', f'algorithm={alg}', KEY])[0])
    assert reason is not None and word in reason and 'il_gail_mixup_step_population' not in reason, (alg, reason)
  assert train.sweep_fallback_reason(_cfgs(['seed=1,2', 'algorithm=GAIL', KEY])[0]) is None   # BCE: as without the key
  assert train.sweep_fallback_reason(_cfgs(['seed=1,2', 'algorithm=SAC', KEY])[0]) is None


def test_the_entry_point_is_bound_exported_and_refuses_on_the_host():
  from imitation_learning_amd import _lib
  assert 'il_gail_mixup_step_population' in _lib._SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), 'il_gail_mixup_step_population')
  assert len(_lib._SIGNATURES['il_gail_mixup_step_population'][1]) == len(_lib._SIGNATURES['il_gail_step_population'][1]) + 3   # + extras_dev, extras_host, mixup_alpha
  assert C.sizeof(_lib.GailExtra) == 32
  assert _lib.lib().il_gail_mixup_step_population(None, None, None, None, 1, None, None, None, 1.0, None) == 1   # IL_ERR_ARG on the host, nothing launched
