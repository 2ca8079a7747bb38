"""Developer tool: one `il_pwil_act_reward_population` launch for L learners against L back-to-back `il_pwil_act_reward` launches, in ONE job on one GPU, interleaved,
5 repeats each. The per-learner entry point is unchanged code: it is the baseline.
  size     every learner on its own 25,000 atoms, D = 24 (HalfCheetah dims with the absorbing bit), time horizon 1,000: 98 chunks of 27 candidates per learner
  post     one pending IL_ACT_REWARD_ON_DEVICE post per learner that no append consumes, so EVERY launch passes the gate and merges (about 25 atoms per launch; the atom
           weights are set back in front of every timed burst, outside the clock, and a burst stays well inside the 1,000 couplings an episode's atoms last)
  time     HIP events around a burst of --burst couplings of all L learners, in stream order: us per coupling of the population = burst time / burst
  check    both forms leave the same atom weights and rewards, bit for bit, after the same number of couplings
The population launch counts as faster only if its median beats the back-to-back median by more than the back-to-back spread (max - min) of this job.
  python profiles/tools/pwil_population_ab.py [--learners 1 4 16] [--burst 200] [--repeats 5] [--out profiles/pwil_population_ab.txt]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import imitation_learning_amd as il
from imitation_learning_amd import _lib
from imitation_learning_amd.acting import NO_ACTION, PENDING, REWARD_ON_DEVICE, _MailboxBlock
from imitation_learning_amd.training import _device_array

ap = argparse.ArgumentParser()
ap.add_argument('--learners', type=int, nargs='+', default=[1, 4, 16])
ap.add_argument('--burst', type=int, default=200)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--out', default=None)
args = ap.parse_args()
assert 1 <= args.burst <= 900, 'a burst must stay inside one episode of 1,000 couplings'
dev = torch.device('cuda', 0)
ATOMS, HORIZON, S, A = 25000, 1000, 18, 6
lines = []


class Cfg(dict):
  __getattr__ = dict.__getitem__


def say(text):
  print(text, flush=True)
  lines.append(text)


def discriminator(seed):
  rs = np.random.RandomState(seed)
  states = (rs.standard_normal((ATOMS, S)) * rs.uniform(0.5, 2.0, S) + rs.standard_normal(S)).astype(np.float32)
  states[:, -1] = 0   # the absorbing bit
  t = dict(states=torch.from_numpy(states), actions=torch.from_numpy(rs.uniform(-1, 1, (ATOMS, A)).astype(np.float32)), rewards=torch.zeros(ATOMS), next_states=torch.from_numpy(states),
           terminals=torch.zeros(ATOMS), timeouts=torch.zeros(ATOMS), weights=torch.ones(ATOMS), num_trajectories=ATOMS // HORIZON)
  return il.PWILDiscriminator(S, A, Cfg(state_only=False, reward_scale=5, reward_bandwidth_scale=5), il.ReplayMemory(ATOMS, S, A, True, transitions=t, device=dev), HORIZON)


class Side:
  """L learners with a pending post each: discriminators, mailboxes, carries (state | action of the pending transition) and the il_pwil_learner array."""

  def __init__(self, L):
    self.L, self.discs = L, [discriminator(100 + l) for l in range(L)]
    self.box = _MailboxBlock(L, S, A)
    rs = np.random.RandomState(7)
    carry = np.zeros((L, S + A + 4), dtype=np.float32)
    carry[:, :S + A] = rs.standard_normal((L, S + A)) * 1.2
    carry[:, S - 1] = 0
    self.carry = torch.from_numpy(carry).to(dev)
    self.box.host[:, 2:6] = (0.0, 0.0, 0.0, 1.0)
    self.box.commit(1, np.full(L, PENDING | NO_ACTION | REWARD_ON_DEVICE, dtype=np.int64))   # never appended: pending at every launch
    base, stride = self.box.tensor.data_ptr(), self.box.floats * 4
    self.mail = [C.c_void_p(base + l * stride) for l in range(L)]
    self.descs = _device_array([_lib.PwilLearner(d._desc, base + l * stride, self.carry[l].data_ptr()) for l, d in enumerate(self.discs)], dev)
    self.shape = self.discs[0]._desc

  def reset(self):
    for d in self.discs: d.reset()

  def population(self, n, st):
    fn, descs, shape = _lib.lib().il_pwil_act_reward_population, _lib.ptr(self.descs), C.byref(self.shape)
    for _ in range(n):
      rc = fn(descs, self.L, shape, st)
      if rc: _lib.check(rc)

  def back_to_back(self, n, st):
    fn = _lib.lib().il_pwil_act_reward
    calls = [(C.byref(d._desc), self.mail[l], _lib.ptr(self.carry[l])) for l, d in enumerate(self.discs)]
    for _ in range(n):
      for desc, mail, carry in calls:
        rc = fn(desc, mail, carry, st)
        if rc: _lib.check(rc)

  def state(self):
    torch.cuda.synchronize()
    return [d.expert_weights.clone() for d in self.discs] + [self.carry.clone()]


def timed(side, form, n):
  side.reset()
  st = torch.cuda.current_stream().cuda_stream
  begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  begin.record()
  getattr(side, form)(n, st)
  end.record()
  end.synchronize()
  return begin.elapsed_time(end) * 1e3 / n   # us per coupling of all L learners


say(f'device {torch.cuda.get_device_name(0)}; PWIL coupling of a pending post against {ATOMS} atoms per learner, D = {S + A}, horizon {HORIZON}; bursts of {args.burst} couplings, '
    f'{args.repeats} interleaved repeats; us per coupling of all L learners (device time between two events)')
FORMS = ('back_to_back', 'population')
verdicts = {}
for L in args.learners:
  side = Side(L)
  got = {}
  for form in FORMS:   # warm-up (code objects), and the check: the same weights, rewards and coupled words after the same number of couplings
    timed(side, form, 20)
    got[form] = side.state()
  assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got['back_to_back'], got['population'])), f'L = {L}: the two forms disagree'
  assert all((w < 0).sum() >= 20 * 20 for w in got['population'][:-1]), 'every launch is meant to merge (about 25 atoms consumed per coupling)'
  us = {form: [] for form in FORMS}
  for _ in range(args.repeats):
    for form in FORMS:   # interleaved: a drift of the machine hits both forms alike
      us[form].append(timed(side, form, args.burst))
  med = {k: float(np.median(v)) for k, v in us.items()}
  spread = max(us['back_to_back']) - min(us['back_to_back'])
  say(f'L = {L} learners (grid {-(-ATOMS // 256)} x {L} workgroups in one launch, against {L} launches of {-(-ATOMS // 256)})')
  for k, v in us.items():
    say(f'  {k:12s}: median {med[k]:8.2f} us  (min {min(v):8.2f} .. max {max(v):8.2f}; repeats ' + ' '.join(f'{r:.2f}' for r in v) + f'); {med[k] / L:.2f} us per learner')
  verdicts[L] = med['back_to_back'] - med['population'] > spread
  say(f'  back_to_back / population = {med["back_to_back"] / med["population"]:.2f}x; the back_to_back spread is {spread:.2f} us: population is '
      f'{"FASTER" if verdicts[L] else "NOT faster"} by more than that')
  del side

if args.out:
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f: f.write('\n'.join(lines) + '\n')
