"""`python train.py -m seed=... algorithm=GMMIL +sweep.schedule=...` without a GPU: which GMMIL sweeps form one population and which run job after job, and why (without
the key a GMMIL sweep runs as it always has: tests/test_sweep_config_cpu.py and tests/test_sweep_red_config_cpu.py pin that); and the layout of the
descriptor the population reward launch indexes on the device (il_gmmil_learner) against the C header. The other algorithms' pins are tests/test_sweep_config_cpu.py and
tests/test_sweep_red_config_cpu.py."""
import ctypes as C
import os
import shutil
import subprocess
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


@pytest.mark.parametrize('argv', [[], ['imitation.mix_expert_data=prefill_memory'], ['optimised_hyperparameters=GMMIL_5_trajectories'], ['optimised_hyperparameters=GMMIL_10_trajectories'],
                                  ['optimised_hyperparameters=GMMIL_25_trajectories'], ['env=ant'], ['imitation.state_only=true'], ['+acting.schedule=fused']],
                         ids=['none', 'prefill_memory', 'GMMIL_5', 'GMMIL_10', 'GMMIL_25', 'ant-D120', 'state_only', 'fused-acting'])
@pytest.mark.parametrize('schedule', ['population', 'per_learner'])
def test_gmmil_seed_sweeps_form_one_population(argv, schedule):
  import train
  cfgs = _cfgs(['seed=1,2,3', 'algorithm=GMMIL', f'+sweep.schedule={schedule}'] + argv)
  assert train.sweep_fallback_reason(cfgs[0]) is None
  assert train.sweep_groups(cfgs) == [([0, 1, 2], None)]


def test_gmmil_population_is_asked_for_with_the_sweep_schedule_key():
  """Without `+sweep.schedule` a GMMIL sweep keeps running job after job, and the reason says how to ask."""
  runs, _ = _groups(['seed=1,2,3', 'algorithm=GMMIL'])
  assert [jobs for jobs, _ in runs] == [[0], [1], [2]]
  assert all('algorithm=GMMIL' in reason and '+sweep.schedule=population|per_learner' in reason and 'il_gmmil_reward_population' in reason for _, reason in runs), runs


def test_the_shipped_gmmil_configurations_train_at_batch_128_without_mixing():
  """What the population launch was sized for: every tuned GMMIL overlay runs batch 128 with mix_expert_data none."""
  for n in (5, 10, 25):
    c = _cfgs(['seed=1,2', 'algorithm=GMMIL', '+sweep.schedule=population', f'optimised_hyperparameters=GMMIL_{n}_trajectories'])[0]
    assert int(c.training.batch_size) == 128 and c.imitation.mix_expert_data == 'none' and not c.imitation.bc_aux_loss


@pytest.mark.parametrize('argv,word', [
    (['imitation.mix_expert_data=mixed_batch'], 'mixed_batch'), (['imitation.bc_aux_loss=true'], 'bc_aux_loss'), (['+acting.schedule=overlap'], 'acting.schedule'),
    (['training.batch_size=100'], 'multiple of 16'), (['reinforcement.actor.depth=3'], 'shape'), (['distributed.world_size=2'], 'world_size')])
def test_gmmil_configurations_without_population_launches_run_job_after_job(argv, word):
  runs, _ = _groups(['seed=1,2', 'algorithm=GMMIL', '+sweep.schedule=population'] + argv)
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  assert all(reason is not None and word in reason for _, reason in runs), runs


def test_gmmil_above_128_dims_runs_job_after_job(monkeypatch):
  """il_gmmil_reward_population is the centred-Gram form (state + action dims <= 128); no D4RL task is wider, so a widened stand-in for `ant` takes its place: 122 + 8 = 130
  dims with actions, 122 without - the same environment under state_only forms a population again."""
  import train
  from imitation_learning_amd import environments
  spec = environments._SPECS['ant']
  monkeypatch.setitem(environments._SPECS, 'ant', (121,) + tuple(spec[1:]))
  assert environments.env_dims('ant', True) == (122, 8) and environments.env_dims('hopper', True) == (12, 3) and environments.env_dims('hopper', False) == (11, 3)
  runs, cfgs = _groups(['seed=1,2', 'algorithm=GMMIL', 'env=ant', '+sweep.schedule=population'])
  assert [jobs for jobs, _ in runs] == [[0], [1]]
  assert all(reason is not None and '130 state + action dims' in reason and '128' in reason for _, reason in runs), runs
  assert train.sweep_fallback_reason(_cfgs(['seed=1,2', 'algorithm=GMMIL', 'env=ant', 'imitation.state_only=true', '+sweep.schedule=population'])[0]) is None
  assert train.sweep_fallback_reason(_cfgs(['seed=1,2', 'algorithm=SAC', 'env=ant'])[0]) is None   # the limit is GMMIL's reward launch's alone


def test_the_fallback_message_of_other_algorithms_lists_gmmil():
  import train
  for alg in ('DRIL', 'PWIL', 'AdRIL'):
    reason = train.sweep_fallback_reason(_cfgs(['seed=1,2', f'algorithm={alg}'])[0])
    assert reason is not None and f'algorithm={alg} has no population launches' in reason and all(a in reason for a in ('SAC', 'GAIL', 'RED', 'GMMIL')), reason


C_PROGRAM = r'''
#include <stddef.h>
#include <stdio.h>
#include "il_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(il_gmmil_learner), offsetof(il_gmmil_learner, policy), offsetof(il_gmmil_learner, expert), offsetof(il_gmmil_learner, gamma_1),
         offsetof(il_gmmil_learner, gamma_2), offsetof(il_gmmil_learner, workspace), offsetof(il_gmmil_learner, out_rewards), sizeof(il_batch));
  return 0;
}
'''


def _c_compiler():
  for cc in (os.environ.get('CC'), 'cc', 'gcc', 'clang', '/opt/rocm/llvm/bin/clang', '/opt/rocm/bin/hipcc'):
    if cc and shutil.which(cc): return shutil.which(cc)
  raise AssertionError('no C compiler found (tried $CC, cc, gcc, clang and the ROCm toolchain that builds the library)')


def test_gmmil_learner_ctypes_mirror_matches_the_header(tmp_path):
  """sizeof and every field offset of _lib.GmmilLearner against a C program compiled with include/il_hip.h, and against the compiled library (il_struct_size(14))."""
  from imitation_learning_amd import _lib
  src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
  src.write_text(C_PROGRAM)
  cc = _c_compiler()
  lang = ['-x', 'c'] if os.path.basename(cc) == 'hipcc' else []
  r = subprocess.run([cc] + lang + ['-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-2000:]
  got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
  G = _lib.GmmilLearner
  assert got == [C.sizeof(G), G.policy.offset, G.expert.offset, G.gamma_1.offset, G.gamma_2.offset, G.workspace.offset, G.out_rewards.offset, C.sizeof(_lib.Batch)], got
  assert got[0] == 2 * C.sizeof(_lib.Batch) + 2 * 4 + 2 * 8 and got[0] % 8 == 0
  assert _lib.lib().il_struct_size(14) == C.sizeof(G)
  ln = G(_lib.Batch(), _lib.Batch(), 0.25, 4.0, 0x1000, 0x2000)   # field order of the constructor the plan uses
  assert (ln.gamma_1, ln.gamma_2, ln.workspace, ln.out_rewards) == (0.25, 4.0, 0x1000, 0x2000)


def test_gmmil_whole_lanes_rule():
  """training.gmmil_whole_lanes is il_gmmil_reward's own rule on host descriptors: pointers 16-byte aligned, leading dimensions and widths multiples of 4, the action side
  exempt under state_only; one learner that does not qualify takes the promise away from all."""
  from imitation_learning_amd import _lib
  from imitation_learning_amd.training import gmmil_whole_lanes
  def b(ps, ls, pa, la):
    x = _lib.Batch(); x.states, x.ld_states, x.actions, x.ld_actions = ps, ls, pa, la
    return x
  ok = b(0x1000, 64, 0x2000, 8)
  assert gmmil_whole_lanes([ok, ok], 56, 8, False) == 1
  assert gmmil_whole_lanes([ok, b(0x1004, 64, 0x2000, 8)], 56, 8, False) == 0 and gmmil_whole_lanes([ok, b(0x1000, 62, 0x2000, 8)], 56, 8, False) == 0
  assert gmmil_whole_lanes([ok], 18, 6, False) == 0 and gmmil_whole_lanes([ok], 56, 6, False) == 0 and gmmil_whole_lanes([ok], 56, 6, True) == 1
  assert gmmil_whole_lanes([b(0x1000, 64, 0x2004, 7)], 56, 8, True) == 1 and gmmil_whole_lanes([b(0x1000, 64, 0x2004, 8)], 56, 8, False) == 0
