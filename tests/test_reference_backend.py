"""`backend=reference` as TEST INFRASTRUCTURE (never imported by the product: tests/test_abi_and_layout.py::test_product_package_never_imports_the_oracle).

BASELINE.json configs[0] is "algorithm=BC env=hopper, 1k iterations on CPU PyTorch reference (plumbing, no GPU)": oracle/ref_bc_config1.py runs exactly that through the
reference's own modules (oracle/_ref, a build product that exists only where the reference does). Its record - initial parameters, parameters after 60 iterations, the
loss of every one of 1,000 iterations - is stored in tests/golden/bc_config1.npz (tests/golden/make_golden.py bc_config1); the expert rows and the batches are rebuilt
from the runner's seeds. The CPU test executes configs[0] as written where oracle/_ref is built and reads the record elsewhere, and replays it on the numpy oracle; the
GPU test feeds the SAME initial parameters and the SAME batches to the HIP path (`il.behavioural_cloning_update`, what train.py's pretraining loop calls: train.py:93-98)
and compares the loss of every one of the first N iterations and the parameters at the end (bounds in the docstring of the GPU test) - the per-step HIP-vs-reference
comparison SURVEY.md 4 asks of the integration level."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, 'oracle', 'ref_bc_config1.py')
RECORD = os.path.join(ROOT, 'tests', 'golden', 'bc_config1.npz')
S, A, H, B, EXPERT_ROWS = 12, 3, 256, 256, 5000   # oracle/ref_bc_config1.py


def _run_reference(tmp_path, iterations):
  out = tmp_path / 'bc_ref.npz'
  r = subprocess.run([sys.executable, RUNNER, '--iterations', str(iterations), '--out', str(out)], capture_output=True, text=True, timeout=600, env=dict(os.environ, HIP_VISIBLE_DEVICES=''))
  assert r.returncode == 0, r.stderr[-2000:]
  return dict(np.load(out))


def _reference_record(iterations):
  """The stored record of oracle/ref_bc_config1.py (seed 0) for `iterations` (60 or 1,000) iterations, with the expert rows and batches rebuilt as the runner draws them."""
  import inputs as gi
  g = np.load(RECORD)
  expert = gi.transitions(np.random.RandomState(100), EXPERT_ROWS, S, A, state_shift=0.5, weighted=True)
  order = np.random.RandomState(200)
  idx = np.stack([order.permutation(EXPERT_ROWS)[:B] for _ in range(iterations)])
  rec = dict(init=g['init'], losses=g['losses'][:iterations], idx=idx, states=expert['states'], actions=expert['actions'], weights=expert['weights'])
  if iterations == 60:
    rec['final'] = g['final_60']
  return rec


def test_baseline_config_1_runs_on_the_cpu_reference(tmp_path):
  """configs[0] as written: 1,000 behavioural-cloning iterations, Hopper dims, CPU, the reference's own code - run live where oracle/_ref is built, its stored record
  elsewhere. Plumbing: finite, and the likelihood of the expert's actions rises. The numpy oracle (oracle/sac.py bc_update) fed the same initial parameters and batches
  follows it: every loss of the first 60 iterations within rtol 2e-5 (measured 2.2e-7); later, float32 rounding differences grow through the chained Adam steps (7 % on
  one 50-iteration mean late in the run), so the mean of the last 200 losses is held to 5 % of the reference's (measured 1.7 %)."""
  from oracle import nets, sac
  live = os.path.isfile(os.path.join(ROOT, 'oracle', '_ref', 'training.pyc'))
  g = _run_reference(tmp_path, 1000) if live else _reference_record(1000)
  ref = g['losses']
  assert ref.shape == (1000,) and np.isfinite(ref).all()
  assert ref[-50:].mean() < ref[:50].mean() - 0.1, (ref[:50].mean(), ref[-50:].mean())
  if live:
    assert np.isfinite(g['final']).all() and not np.array_equal(g['init'], g['final'])
  p = g['init'].copy()
  m, v = np.zeros_like(p), np.zeros_like(p)
  shapes = nets.mlp_shapes(S, H, 2, 2 * A)
  got = np.empty(1000, np.float32)
  for k in range(1000):
    rows = g['idx'][k]
    got[k] = sac.bc_update(p, m, v, k + 1, shapes, A, dict(states=g['states'][rows], actions=g['actions'][rows], weights=g['weights'][rows]), lr=2.5e-4, weight_decay=0)
  assert np.isfinite(p).all() and not np.array_equal(g['init'], p)
  np.testing.assert_allclose(got[:60], ref[:60], rtol=2e-5, err_msg='oracle vs reference: behavioural-cloning loss of the first 60 iterations')
  assert abs(got[-200:].mean() - ref[-200:].mean()) < 0.05 * ref[-200:].mean(), (got[-200:].mean(), ref[-200:].mean())
  assert got[-50:].mean() < got[:50].mean() - 0.1, (got[:50].mean(), got[-50:].mean())


@pytest.mark.gpu
def test_hip_pretraining_follows_the_reference_step_by_step(tmp_path):
  """The first 60 iterations of configs[0] on the HIP path (same initial parameters, same batches): every iteration's loss within rtol 2e-5 (+ 2e-5 of the largest loss)
  of the reference's, the parameters after 60 AdamW steps at the bounds of tests/gpu_util.py."""
  import torch
  import imitation_learning_amd as il
  from gpu_util import DEV, N, T, Cfg, close, close_params
  K = 60
  g = _reference_record(K)
  S, A = 12, 3
  actor = il.SoftActor(S, A, Cfg(hidden_size=256, depth=2, activation='relu'), device=DEV)
  assert actor.flat.numel() == g['init'].size
  actor.flat.copy_(T(g['init']))
  opt = il.AdamW(actor, lr=2.5e-4, weight_decay=0)
  st, ac, w = T(g['states']), T(g['actions']), T(g['weights'])
  losses = []
  for k in range(K):
    rows = torch.from_numpy(g['idx'][k]).to(DEV)
    losses.append(float(il.behavioural_cloning_update(actor, dict(states=st[rows].contiguous(), actions=ac[rows].contiguous(), weights=w[rows].contiguous()), opt)))
  close(np.asarray(losses, np.float32), g['losses'], 'behavioural-cloning loss of every iteration', rtol=2e-5, atol_scale=2e-5)
  # 60 chained AdamW steps: every element within the tight bound + one step per iteration; the fraction outside the tight bound itself grows with the chain (Adam turns
  # ulp-level gradient noise on near-zero gradients into a fraction of a step, tests/gpu_util.py close_params): 1.9e-4 after 1-3 steps (test_bc_update_matches_oracle_and_reference),
  # 3.0e-3 measured after 60 (gpurun_out/r05e), allowed 6e-3
  close_params(N(actor.flat), g['final'], f'actor after {K} pretraining iterations', 2.5e-4, K, outlier_frac=6e-3)
