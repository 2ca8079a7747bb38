"""`python train.py -m seed=... algorithm=RED` without a GPU: which RED sweeps form one population (the reference README's own sweep command among them) and which run
job after job, and why. The other algorithms' pins are tests/test_sweep_config_cpu.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imitation_learning_amd import config  # noqa: E402


def _groups(argv):
  import train
  cfgs, _ = config.compose_multirun(['-m'] + argv)
  for c in cfgs: config.validate(c)
  return train.sweep_groups(cfgs), cfgs


def test_the_readme_sweep_command_forms_one_population():
  """Reference README.md:96-99, word for word."""
  runs, cfgs = _groups(['algorithm=RED', 'optimised_hyperparameters=RED_25_trajectories', 'env=halfcheetah', 'seed=1,2,3,4,5,6,7,8,9,10'])
  assert runs == [(list(range(10)), None)]
  assert [c.seed for c in cfgs] == list(range(1, 11)) and all(c.algorithm == 'RED' and c.env == 'halfcheetah' for c in cfgs)
  d = cfgs[0].imitation.discriminator   # the overlay was applied: depth 2 / tanh / both dropouts is what the population launch must run in eval mode
  assert (int(d.depth), str(d.activation)) == (2, 'tanh') and float(d.dropout) > 0 and cfgs[0].imitation.mix_expert_data == 'none' and not cfgs[0].imitation.bc_aux_loss


@pytest.mark.parametrize('argv', [['algorithm=RED'], ['algorithm=RED', 'imitation.mix_expert_data=prefill_memory'], ['algorithm=RED', '+acting.schedule=fused'],
                                  ['algorithm=RED', 'optimised_hyperparameters=RED_5_trajectories'], ['algorithm=RED', 'optimised_hyperparameters=RED_10_trajectories']],
                         ids=['plain', 'prefill_memory', 'fused-acting', 'RED_5', 'RED_10'])
def test_red_seed_sweeps_form_one_population(argv):
  runs, _ = _groups(['seed=1,2,3'] + argv)
  assert runs == [([0, 1, 2], None)]


@pytest.mark.parametrize('argv,word', [
    (['algorithm=RED', 'imitation.mix_expert_data=mixed_batch'], 'mix_expert_data'), (['algorithm=RED', 'imitation.bc_aux_loss=true'], 'bc_aux_loss'),
    (['algorithm=RED', '+acting.schedule=overlap'], 'acting.schedule'), (['algorithm=RED', 'training.batch_size=100'], 'multiple of 16'),
    (['algorithm=RED', 'reinforcement.actor.depth=3'], 'shape'), (['algorithm=RED', 'distributed.world_size=2'], 'world_size'),
    (['algorithm=DRIL'], 'algorithm=DRIL has no population launches (SAC, GAIL and RED have)')])
def test_red_configurations_without_population_launches_run_job_after_job(argv, word):
  runs, _ = _groups(['seed=1,2'] + argv)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  assert all(reason is not None and word in reason for _, reason in runs), runs


def test_prefill_memory_still_keeps_the_other_algorithms_job_after_job():
  """RED's prefill happens once in front of the loop; the exception is RED's alone."""
  for alg in ('SAC', 'GMMIL'):
    runs, _ = _groups(['seed=1,2', f'algorithm={alg}', 'imitation.mix_expert_data=prefill_memory'])
    assert [jobs for jobs, _ in runs] == [[0], [1]] and all(reason is not None for _, reason in runs), alg
