"""The two tables behind a seed sweep's population, without a GPU and without loading the library: `training.POPULATION_STEPS` (what an algorithm adds to the gathers and
the SAC launches of `BatchedPopulationPlan`) and `train.SWEEP_OPT_INS` (the keys that opt an algorithm's sweeps in, and the reason a sweep without its key is given)."""
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imitation_learning_amd import training  # noqa: E402
from test_sweep_gmmil_config_cpu import _cfgs  # noqa: E402

ALGORITHMS = {'SAC', 'GAIL', 'RED', 'GMMIL', 'DRIL', 'PWIL', 'AdRIL'}


def test_the_step_table_covers_the_algorithms_the_constructor_names():
  assert set(training.POPULATION_STEPS) == ALGORITHMS
  source = inspect.getsource(training.BatchedPopulationPlan.__init__)
  message = re.search(r"'the population launches exist for ([A-Za-z, ]+) learners of one batch size'", source).group(1)
  assert set(re.split(r', | and ', message)) == ALGORITHMS, message
  assert 'p0.algorithm in POPULATION_STEPS' in source   # the assertion that carries the message asks the table


def test_the_steps_with_a_reward_launch_get_the_side_stream():
  """`side` is a second stream exactly where the step has a reward launch to put on it: GAIL (plain and Mixup), RED, GMMIL and DRIL; SAC's, PWIL's and AdRIL's updates are
  one stream's."""
  assert {a for a, step in training.POPULATION_STEPS.items() if step.reward is not None} == {'GAIL', 'RED', 'GMMIL', 'DRIL'}
  source = inspect.getsource(training.BatchedPopulationPlan.__init__)
  assert "self.side = torch.cuda.Stream() if self.step.reward is not None and os.environ.get('IL_POP_OVERLAP', '1') != '0' else None" in source


# what sweep_fallback_reason returned for these sweeps before SWEEP_OPT_INS existed, word for word
REASONS = [
    (['algorithm=PWIL'], 'algorithm=PWIL has no population launches (SAC, GAIL and RED have), and GMMIL under an explicit +sweep.schedule; PWIL trains as one population '
     '(il_pwil_act_reward_population: one coupling launch per lockstep step) only when +sweep.pwil_population=true is given'),
    (['algorithm=AdRIL'], 'algorithm=AdRIL has no population launches (SAC, GAIL and RED have), and GMMIL under an explicit +sweep.schedule; AdRIL trains as one population '
     '(il_batch_mix_relabel_population: one relabel launch per update) only when +sweep.adril_population=true is given'),
    (['algorithm=DRIL'], 'algorithm=DRIL has no population launches (SAC, GAIL and RED have), and GMMIL under an explicit +sweep.schedule; DRIL trains as one population '
     '(il_dril_reward_population, il_bc_step_population) only when +sweep.schedule=population|per_learner is given'),
    (['algorithm=BC'], 'algorithm=BC has no population launches (SAC, GAIL and RED have), and GMMIL under an explicit +sweep.schedule'),
    (['algorithm=GAIL', 'imitation.loss_function=Mixup'], 'imitation.loss_function=Mixup has no population discriminator step (BCE and PUGAIL with an infinite margin have); Mixup '
     "trains as one population (il_gail_mixup_step_population: every learner's coefficients under its own key and counter) only when +sweep.gail_mixup_population=true is given"),
]


def test_the_reasons_built_from_the_opt_in_table_are_the_pinned_texts():
  import train
  for argv, reason in REASONS:
    assert train.sweep_fallback_reason(_cfgs(['seed=1,2'] + argv)[0]) == reason, argv
  assert set(train.SWEEP_OPT_INS) == {'DRIL', 'PWIL', 'AdRIL', 'Mixup'}
  assert [train.SWEEP_OPT_INS[a][0] for a in ('PWIL', 'AdRIL', 'Mixup')] == [train.PWIL_POPULATION_KEY, train.ADRIL_POPULATION_KEY, train.GAIL_MIXUP_POPULATION_KEY]
  for key, (argv, _) in zip((train.PWIL_POPULATION_KEY, train.ADRIL_POPULATION_KEY, '+sweep.schedule=population', None, train.GAIL_MIXUP_POPULATION_KEY), REASONS):
    if key is not None:   # with its key every one of them trains as one population
      cfg = _cfgs(['seed=1,2', key] + argv)[0]
      assert train.sweep_fallback_reason(cfg) is None and train.sweep_opt_in(cfg, key[len('+sweep.'):key.index('=')])
