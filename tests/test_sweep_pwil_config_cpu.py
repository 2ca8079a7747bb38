"""`python train.py -m seed=... algorithm=PWIL +sweep.pwil_population=true` without a GPU: which PWIL sweeps form one population and which run job after job, and why.
The opt-in is a key of its own: without it a PWIL sweep runs as it always has, with or without `+sweep.schedule` (tests/test_sweep_config_cpu.py,
tests/test_sweep_dril_config_cpu.py and tests/test_sweep_gmmil_config_cpu.py pin that text). And the layout of the descriptor the population coupling launch indexes on
the device (il_pwil_learner) against the C header and the compiled library."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imitation_learning_amd import config  # noqa: E402
from test_sweep_gmmil_config_cpu import _c_compiler, _cfgs, _groups  # noqa: E402

KEY = '+sweep.pwil_population=true'


@pytest.mark.parametrize('argv', [[], ['imitation.mix_expert_data=prefill_memory'], ['+acting.schedule=fused'], ['env=halfcheetah'], ['imitation.state_only=true'],
                                  ['imitation.subsample=20'], ['optimised_hyperparameters=PWIL_5_trajectories']],
                         ids=['none', 'prefill_memory', 'fused-acting', 'halfcheetah', 'state_only', 'subsample-20', 'PWIL_5'])
@pytest.mark.parametrize('schedule', [None, 'population', 'per_learner'])
def test_pwil_seed_sweeps_form_one_population_under_the_key(argv, schedule):
  import train
  cfgs = _cfgs(['seed=1,2,3', 'algorithm=PWIL', KEY] + ([f'+sweep.schedule={schedule}'] if schedule else []) + argv)
  assert train.sweep_fallback_reason(cfgs[0]) is None
  assert train.sweep_groups(cfgs) == [([0, 1, 2], None)]
  assert train.sweep_schedule(cfgs[0]) == (schedule or train.SWEEP_DEFAULT_SCHEDULE) and train.SWEEP_DEFAULT_SCHEDULE == 'per_learner'   # the default is not this change's to move


@pytest.mark.parametrize('extra', [[], ['+sweep.schedule=population'], ['+sweep.schedule=per_learner'], ['+sweep.pwil_population=false']], ids=['no-key', 'schedule-population', 'schedule-per_learner', 'key-false'])
def test_pwil_population_is_asked_for_with_a_key_of_its_own(extra):
  """Without `+sweep.pwil_population=true` a PWIL sweep keeps running job after job - `+sweep.schedule` does not opt it in -, the reason keeps its pinned text and says
  how to ask."""
  runs, _ = _groups(['seed=1,2,3', 'algorithm=PWIL'] + extra)
  assert [jobs for jobs, _ in runs] == [[0], [1], [2]]
  for _, reason in runs:
    assert 'algorithm=PWIL has no population launches' in reason and all(a in reason for a in ('SAC', 'GAIL', 'RED', 'GMMIL')), reason
    assert 'il_pwil_act_reward_population' in reason and KEY in reason and 'il_dril_reward_population' not in reason, reason


def test_the_key_opts_no_other_algorithm_in():
  import train
  reason = train.sweep_fallback_reason(_cfgs(['seed=1,2', 'algorithm=AdRIL', KEY])[0])
  assert reason is not None and 'algorithm=AdRIL has no population launches' in reason and 'il_pwil_act_reward_population' not in reason
  assert train.sweep_fallback_reason(_cfgs(['seed=1,2', 'algorithm=DRIL', KEY])[0]) is not None   # DRIL's opt-in stays +sweep.schedule
  assert train.sweep_fallback_reason(_cfgs(['seed=1,2', 'algorithm=SAC', KEY])[0]) is None


@pytest.mark.parametrize('argv,word', [
    (['imitation.mix_expert_data=mixed_batch'], 'mixed_batch'), (['imitation.bc_aux_loss=true'], 'bc_aux_loss'), (['+acting.schedule=overlap'], 'acting.schedule'),
    (['training.batch_size=100'], 'multiple of 16'), (['reinforcement.actor.depth=3'], 'shape'), (['distributed.world_size=2'], 'world_size')])
def test_pwil_configurations_without_population_launches_run_job_after_job(argv, word):
  runs, _ = _groups(['seed=1,2', 'algorithm=PWIL', KEY, '+sweep.schedule=population'] + argv)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  assert all(reason is not None and word in reason for _, reason in runs), runs


@pytest.mark.parametrize('argv,n,horizon,why', [
    (['imitation.trajectories=300', '+synthetic_env.max_episode_steps=10'], 3300, 10, 'm > 256'),         # m = ceil(0.099999 * 3300) + 2 = 332
    (['imitation.trajectories=40'], 40040, 1000, 'G m > 4096'),                                          # m = 42 over 157 chunks
    (['imitation.trajectories=200', '+synthetic_env.max_episode_steps=30', 'imitation.absorbing=false'], 6000, 30, 'G m > 4096')])   # m = 202 over 24 chunks
def test_pwil_atom_sets_outside_the_one_launch_coupling_run_job_after_job(argv, n, horizon, why):
  """The upper bound of a learner's atoms - kept trajectories x horizon / subsample, plus the absorbing rows - against the limits of the one-launch coupling."""
  import math
  import train
  cfgs = _cfgs(['seed=1,2', 'algorithm=PWIL', KEY] + argv)
  assert train.pwil_atoms_upper_bound(cfgs[0]) == (n, horizon)
  m, G = math.ceil((1 / horizon - 1e-6) * n) + 2, -(-n // 256)
  assert (m > 256) if why == 'm > 256' else (m <= 256 and G * m > 4096)
  runs = train.sweep_groups(cfgs)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  assert all('<= 256' in reason and '<= 4096' in reason and str(n) in reason for _, reason in runs), runs


def test_pwil_atom_bound_counts_subsampling_and_absorbing_rows():
  import train
  b = lambda *argv: train.pwil_atoms_upper_bound(_cfgs(['seed=1,2', 'algorithm=PWIL', KEY] + list(argv))[0])
  assert b() == (30 * 1001, 1000)                                                       # the synthetic stand-in's 30 trajectories, one absorbing row each
  assert b('imitation.absorbing=false') == (30 * 1000, 1000)
  assert b('imitation.trajectories=5', 'imitation.subsample=20') == (5 * (51 + 2), 1000)   # every 20th of 1001 rows, and the two absorbing rows the subsampling keeps
  assert b('imitation.trajectories=5', 'imitation.subsample=20', 'imitation.absorbing=false') == (5 * 50, 1000)
  assert b('+synthetic_env.dataset_trajectories=6', '+synthetic_env.max_episode_steps=60') == (6 * 61, 60)


def test_the_bound_covers_what_the_ingest_produces():
  """dataset_to_memory on the synthetic environment, several seeds and subsampling phases: never more rows than the bound."""
  import train
  from imitation_learning_amd import seed as il_seed
  from imitation_learning_amd.environments import make_env
  for sub, absorbing in ((1, True), (7, True), (20, True), (7, False)):
    cfg = _cfgs(['seed=1,2', 'algorithm=PWIL', KEY, f'imitation.subsample={sub}', f'imitation.absorbing={str(absorbing).lower()}', 'imitation.trajectories=4',
                 '+synthetic_env.max_episode_steps=60', '+synthetic_env.dataset_trajectories=6'])[0]
    bound, _ = train.pwil_atoms_upper_bound(cfg)
    for s in (1, 2, 3):
      il_seed(s)
      env = make_env(cfg.env, absorbing, load_data=True, max_episode_steps=60, dataset_trajectories=6)
      env.seed(s)
      mem = env.get_dataset(trajectories=4, subsample=sub, device='cpu')
      assert mem.size <= bound, (sub, absorbing, s, mem.size, bound)


C_PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "il_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(il_pwil_learner), offsetof(il_pwil_learner, d), offsetof(il_pwil_learner, mailbox), offsetof(il_pwil_learner, carry), sizeof(il_pwil));
  return 0;
}
'''


def test_pwil_learner_ctypes_mirror_matches_the_header(tmp_path):
  """sizeof and every field offset of _lib.PwilLearner against a C program compiled with include/il_hip.h, and against the compiled library (il_struct_size(15))."""
  from imitation_learning_amd import _lib
  src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
  src.write_text(C_PROGRAM)
  cc = _c_compiler()
  lang = ['-x', 'c'] if os.path.basename(cc) == 'hipcc' else []
  r = subprocess.run([cc] + lang + ['-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-2000:]
  got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
  P = _lib.PwilLearner
  assert got == [C.sizeof(P), P.d.offset, P.mailbox.offset, P.carry.offset, C.sizeof(_lib.Pwil)], got
  assert got[0] == C.sizeof(_lib.Pwil) + 2 * 8 and got[0] % 8 == 0
  assert _lib.lib().il_struct_size(15) == C.sizeof(P) and _lib.lib().il_struct_size(4) == C.sizeof(_lib.Pwil) and _lib.lib().il_struct_size(16) == -1
  d = _lib.Pwil(600, 15, 12, 3, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 5.0, 2.5, 0.024999)
  ln = P(d, 0x6000, 0x7000)   # field order of the constructor the worker uses; the descriptor is copied, not referenced
  d.n_atoms = 1
  assert (ln.d.n_atoms, ln.d.dists, ln.d.agent_weight, ln.mailbox, ln.carry) == (600, 0x3000, 0.024999, 0x6000, 0x7000)
