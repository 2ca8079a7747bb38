"""Developer tool: one `il_gail_mixup_step_population` for L Mixup discriminators against L back-to-back per-learner sequences (`il_noise_fill_beta` for alpha != 1,
`il_gail_disc_step`, `il_gail_reward`), in ONE job on one GPU, interleaved, 5 repeats each. The per-learner entry points are unchanged code: they are the baseline.
  shapes   the two tuned Mixup overlays' discriminators at HalfCheetah dims with the absorbing bit (S = 18, A = 6), hidden 64, depth 1:
             GAIL_5   batch 1024, spectral norm on,  entropy bonus 0.24, gradient penalty 0.28
             GAIL_10  batch 512,  spectral norm off, entropy bonus 0.025, gradient penalty 0.44
  alpha    1 (coefficients on chip) and 0.5 (one coefficient launch for all learners against one il_noise_fill_beta per learner)
  time     HIP events around a burst of --burst steps of all L learners, in stream order: us per step of the population = burst time / burst
  check    both forms leave the same parameters and rewards, bit for bit, after the first step
The population launches count as faster only if their median beats the back-to-back median by more than the back-to-back spread (max - min) of this job.
  python profiles/tools/gail_mixup_population_ab.py [--shape GAIL_5 GAIL_10] [--alpha 1 0.5] [--learners 1 4 16] [--burst 200] [--repeats 5] [--out profiles/gail_mixup_population_ab.txt]
--out appends, so that a job may run one (shape, alpha) per process, each under its own time limit."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import imitation_learning_amd as il
from imitation_learning_amd import _lib
from imitation_learning_amd import training as il_training
from imitation_learning_amd.memory import batch_desc
from imitation_learning_amd.training import _device_array

SHAPES = {'GAIL_5': dict(B=1024, sn=True, ent=0.24145587952807546, gp=0.2799364347010851), 'GAIL_10': dict(B=512, sn=False, ent=0.024794470891356467, gp=0.4359957529231906)}
ap = argparse.ArgumentParser()
ap.add_argument('--shape', nargs='+', default=['GAIL_5', 'GAIL_10'], choices=sorted(SHAPES))
ap.add_argument('--alpha', type=float, nargs='+', default=[1.0, 0.5])
ap.add_argument('--learners', type=int, nargs='+', default=[1, 4, 16])
ap.add_argument('--burst', type=int, default=200)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda', 0)
S, A, H = 18, 6, 64
lines = []


class Cfg(dict):
  __getattr__ = dict.__getitem__


def say(text):
  print(text, flush=True)
  lines.append(text)


class Side:
  """L learners: own discriminator, AdamW state, Philox key and counter, batches, reward and coefficient buffers, and the device arrays the population call indexes."""

  def __init__(self, L, shape, alpha):
    self.L, self.alpha, B = L, alpha, shape['B']
    icfg = Cfg(state_only=False, spectral_norm=shape['sn'], loss_function='Mixup', grad_penalty=shape['gp'], entropy_bonus=shape['ent'], mixup_alpha=alpha, pos_class_prior=0.7,
               nonnegative_margin=float('inf'), discriminator=Cfg(hidden_size=H, depth=1, activation='relu', reward_shaping=False, subtract_log_policy=False, reward_function='AIRL'))
    self.ln = []
    for l in range(L):
      torch.manual_seed(7 + l)
      rs = np.random.RandomState(7 + l)
      disc = il.GAILDiscriminator(S, A, icfg, 0.97, device=dev)
      opt = il.AdamW(disc, lr=3e-5, weight_decay=10)
      d = il_training.disc_descriptor(disc, B, opt, icfg, tag=('gail-mixup-ab', id(self), l))
      ctr = torch.tensor([3 + l], dtype=torch.int32, device=dev)
      d.noise_seed, d.noise_counter = 1234 + 7919 * l, ctr.data_ptr()
      batch = lambda shift: {k: torch.from_numpy(v).to(dev) for k, v in dict(
          states=(rs.standard_normal((B, S)) + shift).astype(np.float32), actions=rs.uniform(-1, 1, (B, A)).astype(np.float32), rewards=np.zeros(B, np.float32),
          next_states=(rs.standard_normal((B, S)) + shift).astype(np.float32), terminals=np.zeros(B, np.float32), weights=np.ones(B, np.float32), absorbing=np.zeros(B, np.float32)).items()}
      pol, exp = batch(0.0), batch(0.5)
      eps, rewards = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
      self.ln.append(dict(disc=disc, opt=opt, d=d, ctr=ctr, pol=pol, exp=exp, pb=batch_desc(pol), eb=batch_desc(exp), eps=eps, rewards=rewards, extra=_lib.GailExtra(eps_mix=eps.data_ptr()),
                          fresh=(disc.flat.clone(), disc.sn.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count.clone())))
    self.descs, self.pols, self.exps = (_device_array([x[k] for x in self.ln], dev) for k in ('d', 'pb', 'eb'))
    self.reward_ptrs = torch.tensor([x['rewards'].data_ptr() for x in self.ln], dtype=torch.int64, device=dev)
    self.extras_host = (_lib.GailExtra * L)(*[x['extra'] for x in self.ln])
    self.extras = _device_array([x['extra'] for x in self.ln], dev)

  def reset(self):
    for x in self.ln:
      for t, f in zip((x['disc'].flat, x['disc'].sn, x['opt'].exp_avg, x['opt'].exp_avg_sq, x['opt'].step_count), x['fresh']): t.copy_(f)

  def population(self, n, st):
    fn, given = _lib.lib().il_gail_mixup_step_population, self.alpha != 1.0
    a = (_lib.ptr(self.descs), _lib.ptr(self.pols), _lib.ptr(self.exps), _lib.ptr(self.reward_ptrs), self.L, C.byref(self.ln[0]['d']), _lib.ptr(self.extras) if given else None,
         C.cast(self.extras_host, C.c_void_p) if given else None, self.alpha, st)
    for _ in range(n):
      rc = fn(*a)
      if rc: _lib.check(rc)

  def back_to_back(self, n, st):
    L_, given = _lib.lib(), self.alpha != 1.0
    for _ in range(n):
      for x in self.ln:
        d = x['d']
        if given:
          rc = L_.il_noise_fill_beta(C.c_uint64(d.noise_seed), _lib.ptr(x['ctr']), self.alpha, x['eps'].numel(), _lib.ptr(x['eps']), st)
          if rc: _lib.check(rc)
        rc = L_.il_gail_disc_step(C.byref(d), C.byref(x['pb']), C.byref(x['eb']), None, C.byref(x['extra']) if given else None, 0, st)
        if rc: _lib.check(rc)
        rc = L_.il_gail_reward(C.byref(d), C.byref(x['pb']), _lib.ptr(x['rewards']), None, None, st)
        if rc: _lib.check(rc)


def timed(side, form, n):
  st = torch.cuda.current_stream().cuda_stream
  begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  begin.record()
  getattr(side, form)(n, st)
  end.record()
  end.synchronize()
  return begin.elapsed_time(end) * 1e3 / n   # us per step of all L learners


FORMS = ('back_to_back', 'population')
say(f'device {torch.cuda.get_device_name(0)}; Mixup discriminator step + relabel, S = {S}, A = {A}, hidden {H}; bursts of {args.burst} steps, {args.repeats} interleaved repeats; '
    f'us per step of all L learners (device time between two events)')
for name in args.shape:
  shape = SHAPES[name]
  for alpha in args.alpha:
    for L in args.learners:
      side = Side(L, shape, alpha)
      got = {}
      for form in FORMS:   # the check, and the warm-up (code objects)
        side.reset()
        getattr(side, form)(1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got[form] = [(torch.cat([x['disc'].flat, x['disc'].sn]), x['rewards'].clone()) for x in side.ln]
      for l, ((pa, ra), (pb, rb)) in enumerate(zip(got['back_to_back'], got['population'])):
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)) and torch.equal(ra.view(torch.int32), rb.view(torch.int32)), f'{name}, alpha {alpha}, L = {L}: learner {l}: the two forms disagree'
      for form in FORMS: timed(side, form, 20)
      us = {form: [] for form in FORMS}
      for _ in range(args.repeats):
        for form in FORMS:   # interleaved: a drift of the machine hits both forms alike
          us[form].append(timed(side, form, args.burst))
      med = {k: float(np.median(v)) for k, v in us.items()}
      spread = max(us['back_to_back']) - min(us['back_to_back'])
      per = (1 if alpha != 1.0 else 0) + 3
      say(f'{name} (batch {shape["B"]}, spectral norm {"on" if shape["sn"] else "off"}), alpha {alpha:g}, L = {L} learners ({per} launches against {per * L})')
      for k, v in us.items():
        say(f'  {k:12s}: median {med[k]:8.2f} us  (min {min(v):8.2f} .. max {max(v):8.2f}; repeats ' + ' '.join(f'{r:.2f}' for r in v) + f'); {med[k] / L:.2f} us per learner')
      faster = med['back_to_back'] - med['population'] > spread
      say(f'  back_to_back / population = {med["back_to_back"] / med["population"]:.2f}x; the back_to_back spread is {spread:.2f} us: population is '
          f'{"FASTER" if faster else "NOT faster"} by more than that')
      del side

if args.out:
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'a') as f: f.write('\n'.join(lines) + '\n')
