"""Developer tool: one `il_batch_mix_relabel_population` launch for L learners against L back-to-back `il_batch_mix_relabel_dyn` launches, in ONE job on one GPU,
interleaved, 5 repeats each. The per-learner entry point is unchanged code: it is the baseline.
  size     every learner on its own batch of 512 rows at HalfCheetah dims with the absorbing bit (S = 18, A = 6: rows of 48 floats), AdRIL (label 2, update_freq 1250)
  turn     a balanced learner's expert turn (n_expert = n): every row is copied from the expert batch, the full-copy case. The launch is idempotent on such a turn, so a
           burst repeats it without setting anything back
  time     HIP events around a burst of --burst relabels of all L learners, in stream order: us per relabel of the population = burst time / burst
  check    both forms leave the same rows, bit for bit, on an expert turn, a policy turn and a half-and-half batch
The population launch counts as faster only if its median beats the back-to-back median by more than the back-to-back spread (max - min) of this job.
  python profiles/tools/adril_population_ab.py [--learners 1 4 16] [--batch 512] [--burst 500] [--repeats 5] [--out profiles/adril_population_ab.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from imitation_learning_amd import _lib
from imitation_learning_amd.training import _device_array

ap = argparse.ArgumentParser()
ap.add_argument('--learners', type=int, nargs='+', default=[1, 4, 16])
ap.add_argument('--batch', type=int, default=512)
ap.add_argument('--burst', type=int, default=500)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda', 0)
S, A, LABEL, UPDATE_FREQ, B = 18, 6, 2, 1250, args.batch
ROW = int(_lib.lib().il_ring_row_floats(S, A))
lines = []


def say(text):
  print(text, flush=True)
  lines.append(text)


class Side:
  """L learners: own policy rows (stamps over three rounds), expert rows, dyn words (row l of one (L, 3) tensor), reward_expert, and the il_mix_learner array."""

  def __init__(self, L):
    rs = np.random.RandomState(11)
    self.L = L
    pol = rs.standard_normal((L, B, ROW)).astype(np.float32)
    pol[:, :, 2 * S + A + 4] = rs.randint(1, 3800, (L, B))
    self.fresh = torch.from_numpy(pol).to(dev)
    self.rows = self.fresh.clone()
    self.erows = torch.from_numpy((rs.standard_normal((L, B, ROW)) + 3).astype(np.float32)).to(dev)
    self.dyn = torch.zeros((L, 3), dtype=torch.int64, device=dev)
    self.reward = [float(np.float32(1 / (5 + l))) for l in range(L)]
    self.descs = _device_array([_lib.MixLearner(self.rows[l].data_ptr(), self.erows[l].data_ptr(), self.dyn[l].data_ptr(), self.reward[l]) for l in range(L)], dev)

  def turn(self, n_expert):
    self.rows.copy_(self.fresh)
    self.dyn.copy_(torch.tensor([[n_expert, 3, 4 + l] for l in range(self.L)], dtype=torch.int64))

  def population(self, n, st):
    fn, descs = _lib.lib().il_batch_mix_relabel_population, _lib.ptr(self.descs)
    for _ in range(n):
      rc = fn(descs, self.L, B, S, A, LABEL, UPDATE_FREQ, st)
      if rc: _lib.check(rc)

  def back_to_back(self, n, st):
    fn = _lib.lib().il_batch_mix_relabel_dyn
    calls = [(_lib.ptr(self.rows[l]), _lib.ptr(self.erows[l]), self.reward[l], _lib.ptr(self.dyn[l])) for l in range(self.L)]
    for _ in range(n):
      for rows, erows, reward, dyn in calls:
        rc = fn(rows, erows, B, S, A, LABEL, UPDATE_FREQ, reward, dyn, st)
        if rc: _lib.check(rc)


def timed(side, form, n):
  st = torch.cuda.current_stream().cuda_stream
  begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  begin.record()
  getattr(side, form)(n, st)
  end.record()
  end.synchronize()
  return begin.elapsed_time(end) * 1e3 / n   # us per relabel of all L learners


say(f'device {torch.cuda.get_device_name(0)}; AdRIL mix + relabel of a balanced expert turn (n_expert = n = {B}: every row copied), S = {S}, A = {A}, rows of {ROW} floats; bursts of '
    f'{args.burst} relabels, {args.repeats} interleaved repeats; us per relabel of all L learners (device time between two events)')
FORMS = ('back_to_back', 'population')
for L in args.learners:
  side = Side(L)
  for n_expert in (0, B // 2, B):   # the check, and the warm-up (code objects); the last one leaves the timed turn staged
    got = {}
    for form in FORMS:
      side.turn(n_expert)
      getattr(side, form)(1, torch.cuda.current_stream().cuda_stream)
      torch.cuda.synchronize()
      got[form] = side.rows.clone()
    assert torch.equal(got['back_to_back'].view(torch.int32), got['population'].view(torch.int32)), f'L = {L}, n_expert = {n_expert}: the two forms disagree'
    assert not torch.equal(got['population'], side.fresh)
  for form in FORMS: timed(side, form, 50)
  us = {form: [] for form in FORMS}
  for _ in range(args.repeats):
    for form in FORMS:   # interleaved: a drift of the machine hits both forms alike
      us[form].append(timed(side, form, args.burst))
  med = {k: float(np.median(v)) for k, v in us.items()}
  spread = max(us['back_to_back']) - min(us['back_to_back'])
  lanes = B * ROW // 4
  say(f'L = {L} learners (grid {-(-lanes // 256)} x {L} workgroups of 16-byte lanes in one launch, against {L} launches of {-(-B * ROW // 256)} workgroups of floats)')
  for k, v in us.items():
    say(f'  {k:12s}: median {med[k]:8.2f} us  (min {min(v):8.2f} .. max {max(v):8.2f}; repeats ' + ' '.join(f'{r:.2f}' for r in v) + f'); {med[k] / L:.2f} us per learner')
  faster = med['back_to_back'] - med['population'] > spread
  say(f'  back_to_back / population = {med["back_to_back"] / med["population"]:.2f}x; the back_to_back spread is {spread:.2f} us: population is '
      f'{"FASTER" if faster else "NOT faster"} by more than that')
  del side

if args.out:
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f: f.write('\n'.join(lines) + '\n')
