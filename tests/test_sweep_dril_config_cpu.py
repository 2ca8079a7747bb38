"""`python train.py -m seed=... algorithm=DRIL [+sweep.schedule=...]` without a GPU: which DRIL sweeps form one population and which run job after job, and why. Without the
key a DRIL sweep runs as it always has (tests/test_sweep_red_config_cpu.py and tests/test_sweep_gmmil_config_cpu.py pin that reason); with it, the shipped configuration
(bc_aux_loss on) and the three tuned overlays train as one population. The population launches take no new descriptor struct (il_dril and il_sac as they are), so there is
no layout to check here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imitation_learning_amd import config  # noqa: E402


def _cfgs(argv):
  cfgs, _ = config.compose_multirun(['-m'] + argv)
  for c in cfgs: config.validate(c)
  return cfgs


def _groups(argv):
  import train
  cfgs = _cfgs(argv)
  return train.sweep_groups(cfgs), cfgs


@pytest.mark.parametrize('argv', [[], ['imitation.bc_aux_loss=false'], ['imitation.mix_expert_data=prefill_memory'], ['+acting.schedule=fused'],
                                  ['imitation.bc_aux_loss=false', 'imitation.mix_expert_data=prefill_memory']],
                         ids=['shipped-bc_aux', 'no-bc_aux', 'prefill_memory', 'fused-acting', 'no-bc_aux-prefill'])
@pytest.mark.parametrize('schedule', ['population', 'per_learner'])
def test_dril_seed_sweeps_form_one_population_under_the_key(argv, schedule):
  import train
  cfgs = _cfgs(['seed=1,2,3', 'algorithm=DRIL', f'+sweep.schedule={schedule}'] + argv)
  assert train.sweep_fallback_reason(cfgs[0]) is None
  assert train.sweep_groups(cfgs) == [([0, 1, 2], None)]


def test_the_shipped_dril_configuration_sets_the_bc_auxiliary_loss():
  """What il_bc_step_population was built for: conf/algorithm/DRIL.yaml sets bc_aux_loss, and no tuned overlay takes it back."""
  for extra in ([], ['optimised_hyperparameters=DRIL_5_trajectories'], ['optimised_hyperparameters=DRIL_10_trajectories'], ['optimised_hyperparameters=DRIL_25_trajectories']):
    c = _cfgs(['seed=1,2', 'algorithm=DRIL', '+sweep.schedule=population'] + extra)[0]
    assert bool(c.imitation.bc_aux_loss) and c.imitation.mix_expert_data == 'none' and int(c.training.batch_size) % 16 == 0, extra


@pytest.mark.parametrize('n', [5, 10, 25])
def test_the_shipped_dril_overlays_form_one_population_under_the_key(n):
  runs, cfgs = _groups(['seed=1,2,3,4', 'algorithm=DRIL', f'optimised_hyperparameters=DRIL_{n}_trajectories', '+sweep.schedule=population'])
  assert runs == [([0, 1, 2, 3], None)]
  d = cfgs[0].imitation.discriminator
  assert int(d.depth) in (1, 2) and str(d.activation) in ('tanh', 'relu') and int(d.hidden_size) <= 256 and int(d.hidden_size) % 2 == 0   # inside il_dril_reward_population's limits


def test_dril_population_is_asked_for_with_the_sweep_schedule_key():
  """Without `+sweep.schedule` a DRIL sweep keeps running job after job; the reason keeps the substrings other tests pin and says how to ask."""
  runs, _ = _groups(['seed=1,2,3', 'algorithm=DRIL'])
  assert [jobs for jobs, _ in runs] == [[0], [1], [2]]
  for _, reason in runs:
    assert 'algorithm=DRIL has no population launches (SAC, GAIL and RED have)' in reason and all(a in reason for a in ('SAC', 'GAIL', 'RED', 'GMMIL')), reason
    assert '+sweep.schedule=population|per_learner' in reason and 'il_dril_reward_population' in reason and 'il_bc_step_population' in reason, reason


@pytest.mark.parametrize('argv,word', [
    (['imitation.mix_expert_data=mixed_batch'], 'mixed_batch'), (['reinforcement.actor.depth=3'], 'shape'), (['reinforcement.actor.hidden_size=320', 'reinforcement.critic.hidden_size=320'], 'shape'),
    (['training.batch_size=100'], 'multiple of 16'), (['distributed.world_size=2'], 'world_size'), (['+acting.schedule=overlap'], 'acting.schedule')])
@pytest.mark.parametrize('schedule', ['population', 'per_learner'])
def test_dril_configurations_without_population_launches_run_job_after_job(argv, word, schedule):
  runs, _ = _groups(['seed=1,2', 'algorithm=DRIL', f'+sweep.schedule={schedule}'] + argv)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  assert all(reason is not None and word in reason for _, reason in runs), runs


@pytest.mark.parametrize('alg', ['GAIL', 'RED', 'GMMIL', 'SAC'])
@pytest.mark.parametrize('key', [[], ['+sweep.schedule=population']], ids=['no-key', 'explicit-schedule'])
def test_the_bc_auxiliary_loss_still_keeps_the_other_algorithms_job_after_job(alg, key):
  """il_bc_step_population is wired up for DRIL alone: bc_aux_loss sweeps of the other algorithms keep their reason (GMMIL: under an explicit schedule too)."""
  runs, _ = _groups(['seed=1,2', f'algorithm={alg}', 'imitation.bc_aux_loss=true'] + key)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  want = 'il_gmmil_reward_population' if (alg == 'GMMIL' and not key) else 'bc_aux_loss'
  assert all(reason is not None and want in reason for _, reason in runs), runs


def test_the_other_algorithms_without_population_launches_are_not_opted_in_by_the_key():
  import train
  for alg in ('PWIL', 'AdRIL'):
    reason = train.sweep_fallback_reason(_cfgs(['seed=1,2', f'algorithm={alg}', '+sweep.schedule=population'])[0])
    assert reason is not None and f'algorithm={alg} has no population launches' in reason and 'il_dril_reward_population' not in reason, reason
