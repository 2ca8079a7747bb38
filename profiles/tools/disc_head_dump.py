#!/usr/bin/env python3
"""Two updates and one reward call of each adversarial discriminator (il_gail_disc / il_gail_shaped / il_gail_deep / il_gail_shaped_deep _step and _reward), every result
written as .npy: a refactor that claims the same bits runs this against both trees / both libraries and compares the directories byte for byte.

  python profiles/tools/disc_head_dump.py OUT_DIR [--emu] [--root TREE] [--only V.CASE,..]  run; TREE (default: this checkout) is where the package, tests/golden/inputs.py and, with
                                                                            --emu, tests/host_emu come from. Without --emu: the GPU, libil_hip.so or IL_HIP_LIBRARY.
  python profiles/tools/disc_head_dump.py --compare DIR_A DIR_B             exit status 1 unless both hold the same files with the same bytes

Cases: BCE + gradient penalty + entropy bonus, PUGAIL with an infinite margin, PUGAIL with a finite margin on both sides of the clamp (prior 0.5: V < 0, so margin 0
clamps and margin 10 does not), Mixup with given draws and an entropy bonus, subtract_log_policy offsets (two-batch and mixed), and a ragged batch (33 rows for the
32-row kernel, 72 for the 16-row ones). Networks: torch's own initialisation under a fixed seed (so construction is compared too); batches: tests/golden/inputs.py."""
import filecmp, os, sys

if len(sys.argv) == 4 and sys.argv[1] == '--compare':
  a, b = sys.argv[2:]
  fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
  bad = [f for f in fa if f not in fb or not filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False)] + [f for f in fb if f not in fa]
  print(f'{len(fa)} / {len(fb)} files, {len(bad)} differ' + ''.join('\n  ' + f for f in bad))
  sys.exit(1 if bad or not fa else 0)

args = [a for i, a in enumerate(sys.argv) if i and not a.startswith('--') and sys.argv[i - 1] not in ('--root', '--only')]
emu = '--emu' in sys.argv
root = os.path.abspath(sys.argv[sys.argv.index('--root') + 1] if '--root' in sys.argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
out_dir = os.path.abspath(args[0]); os.makedirs(out_dir, exist_ok=True)
only = sys.argv[sys.argv.index('--only') + 1].split(',') if '--only' in sys.argv else None   # e.g. --only gail_shaped.mixup,gail.bce
sys.path[:0] = [root, os.path.join(root, 'tests'), os.path.join(root, 'tests', 'golden')]

import ctypes as C
import numpy as np
import torch
import imitation_learning_amd as il
from imitation_learning_amd import _lib, training
import inputs

DEV = 'cuda'
if emu:   # the kernel sources on the host (tests/host_emu): its entry points in front of the real library's host-side functions, CPU tensors let through
  from host_emu import build as emu_build
  handle, real = emu_build.load(), _lib.lib()

  class Facade:
    def __getattr__(self, name):
      try:
        fn = getattr(handle, name)
      except AttributeError:
        return getattr(real, name)
      fn.restype, fn.argtypes = _lib._SIGNATURES[name]
      return fn

  _lib._lib, _lib.stream_ptr, _lib.on_device, DEV = Facade(), (lambda: None), (lambda t: True), 'cpu'


class Cfg(dict):
  __getattr__ = dict.__getitem__


class Actor:   # subtract_log_policy asks the actor for log pi(a|s) only: a fixed function of the rows
  @staticmethod
  def log_prob(s, a):
    return (-0.5 * (a * a).sum(1) - 0.1 * s[:, 0] - 1.0).contiguous()


T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
VARIANTS = dict(gail=dict(shaping=False, depth=1, activation='relu', ragged=72), gail_shaped=dict(shaping=True, depth=1, activation='relu', ragged=33),
                gail_deep=dict(shaping=False, depth=2, activation='tanh', ragged=72), gail_shaped_deep=dict(shaping=True, depth=2, activation='tanh', ragged=72))
CASES = dict(   # loss_function, (prior, margin), grad_penalty, entropy_bonus, subtract_log_policy, batch (None: the variant's ragged one)
    bce=('BCE', (0.0, float('inf')), 0.7, 0.02, False, 64), pugail_inf=('PUGAIL', (0.5, float('inf')), 1.0, 0.0, False, 80),
    pugail_clamped=('PUGAIL', (0.5, 0.0), 0.5, 0.01, False, 64), pugail_open=('PUGAIL', (0.5, 10.0), 0.5, 0.01, False, 64),
    mixup=('Mixup', (0.0, float('inf')), 0.3, 0.05, False, 80), bce_logp=('BCE', (0.0, float('inf')), 0.0, 0.0, True, 64),
    mixup_logp=('Mixup', (0.0, float('inf')), 0.4, 0.0, True, 64), ragged=('PUGAIL', (0.5, 10.0), 0.6, 0.03, False, None))
S, A, STEPS = inputs.DIMS['hopper'] + (2,)

count = 0
for vi, (vname, v) in enumerate(VARIANTS.items()):
  for ci, (cname, (loss, (prior, margin), gp, eb, sub, B)) in enumerate(CASES.items()):
    if only and f'{vname}.{cname}' not in only: continue
    B = B or v['ragged']
    icfg = Cfg(state_only=False, spectral_norm=ci % 2 == 0, loss_function=loss, pos_class_prior=prior, nonnegative_margin=margin, grad_penalty=gp, entropy_bonus=eb, mixup_alpha=0.7,
               discriminator=Cfg(hidden_size=32 + 16 * (ci % 3), depth=v['depth'], activation=v['activation'], reward_shaping=v['shaping'], subtract_log_policy=sub, reward_function=('AIRL', 'GAIL', 'FAIRL')[ci % 3]))
    torch.manual_seed(1000 + 10 * vi + ci)
    d = il.GAILDiscriminator(S, A, icfg, 0.97, device=DEV)
    assert type(d).__name__ == dict(gail='GAILDiscriminator', gail_shaped='ShapedGAILDiscriminator', gail_deep='DeepGAILDiscriminator', gail_shaped_deep='ShapedDeepGAILDiscriminator')[vname]
    opt = il.AdamW(d, lr=1e-3, weight_decay=0.1)
    rs = np.random.RandomState(7000 + 10 * vi + ci)
    res = {'flat0': d.flat.clone(), 'sn0': d.sn.clone()}
    for k in range(STEPS):
      pol = {n: T(x) for n, x in inputs.transitions(rs, B, S, A, weighted=True, terminal_frac=0.3).items()}
      exp = {n: T(x) for n, x in inputs.transitions(rs, B, S, A, state_shift=0.5, weighted=True, terminal_frac=0.3).items()}
      eps_gp, eps_mix = T(rs.uniform(size=B).astype(np.float32)), T(rs.beta(0.7, 0.7, size=B).astype(np.float32))
      training.adversarial_imitation_update(Actor, d, pol, exp, opt, icfg, eps_gp=eps_gp, eps_mix=eps_mix if loss == 'Mixup' else None)
      res.update({f'flat{k + 1}': d.flat.clone(), f'grad{k + 1}': opt.grad.clone(), f'm{k + 1}': opt.exp_avg.clone(), f'v{k + 1}': opt.exp_avg_sq.clone(), f'sn{k + 1}': d.sn.clone()})
    gi = il.make_gail_input(pol['states'], pol['actions'], pol['next_states'], pol['terminals'], Actor, v['shaping'], sub)
    res['rewards'], res['logits'] = d.predict_reward(**gi), d(**gi)
    if DEV == 'cuda': torch.cuda.synchronize()
    for n, t in res.items():
      np.save(os.path.join(out_dir, f'{vname}.{cname}.{n}.npy'), t.detach().cpu().numpy()); count += 1
    assert all(bool(torch.isfinite(t).all()) for t in res.values()), (vname, cname)
print(f'{count} arrays of {len(VARIANTS) * len(CASES)} cases -> {out_dir}')
