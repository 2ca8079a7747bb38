"""Developer tool: per-phase durations of the policy / critic launch (k_policy_critic_pair or k_policy_critic_quad, whichever the build and IL_QUAD select) in ONE steady-state
SAC+GAIL update of the headline schedule, from a -DIL_TIMELINE build:

  bash profiles/tools/build_variants.sh tl:"-DIL_TIMELINE -w"
  IL_HIP_LIBRARY=variants/tl/libil_hip.so python profiles/tools/quad_timeline.py [replays]

The critic workgroups stamp slots 0 .. 7 of timeline kernel 11 (launched, prologue requested, layer 1 done, layer 2 done + published, the other parts' h2 received, slot 5,
layer 2 backward done, arrival signalled); the helpers stamp kernel 3. Slot 5: in the quad launch "Q stored", stamped by thread 256 of quarter 0 alone (its waves 4 .. 7 sum
Q beside the backward; the mask is written at the hop) - the other quarters leave it 0 and the row is over quarter 0's workgroups; in the pair launch, and in builds of
the quad from before the mask moved to the hop, every workgroup's "Q + mask done", between the hop and the backward. Per-phase durations are per workgroup (one slot to the next), then min / median / max over
the critic workgroups of the last replay; absolute times are microseconds after the launch's first workgroup started."""
import ctypes as C
import sys
sys.path.insert(0, '.')
import numpy as np, torch, bench
from imitation_learning_amd import _lib

K, W, S = 12, 512, 8   # IL_TL_K, IL_TL_WGS, IL_TL_SLOTS (csrc/il_common.hpp)
dev = torch.device('cuda', 0)
plan, nets, _ = bench.build(dev, 0)
plan.capture(warmup=3)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
for _ in range(n): plan.replay()
torch.cuda.synchronize()
assert plan.sync_timeouts() == 0
raw = C.CDLL(_lib.LIB_PATH)
buf = (C.c_ulonglong * (K * W * S))()
assert raw.il_debug_timeline_sac(buf) == 0
sac = np.frombuffer(buf, dtype=np.uint64).reshape(K, W, S).astype(np.int64)
nt = plan.B // 16
p = sac[11]
last = p[:, 7].max()
live = (p[:, 0] > 0) & (p[:, 0] >= last - 20000)   # the last replay's critic workgroups (within 200 us of its last arrival)
ncw = int(live[:8 * nt].sum())
parts = 4 if ncw >= 8 * nt else 2
c = p[:2 * parts * nt]
t0 = c[:, 0].min()
us = lambda a: (np.asarray(a, np.float64)) / 100.0


def row(name, a):
  a = np.asarray(a, np.float64)
  print(f'  {name:44s} {a.min():7.2f} {np.median(a):7.2f} {a.max():7.2f}')


print(f'B = {plan.B}; {"QUAD" if parts == 4 else "PAIR"} mode ({2 * parts * nt} critic workgroups); us: min / median / max over them')
print('durations')
for lo, hi, name in ((0, 1, 'prologue (rows, W1, panel requested)'), (1, 2, 'layer 1'), (2, 3, 'layer 2 forward + publish'), (3, 4, 'hop (other parts received)'),
                     (4, 6, 'received -> layer 2 backward done'), (6, 7, 'dQ/da partials + arrival')):
  row(name, us(c[:, hi] - c[:, lo]))
qs = c[c[:, 5] >= c[:, 4]]   # (a slot 5 of this replay)
if len(qs): row(f'received -> slot 5 ({len(qs)} workgroups: Q stored / Q + mask)', us(qs[:, 5] - qs[:, 4]))
row('whole critic workgroup', us(c[:, 7] - c[:, 0]))
print('absolute (after the first critic workgroup started)')
for s, name in ((2, 'layer 1 done'), (3, 'layer 2 forward done'), (4, 'received'), (6, 'layer 2 backward done'), (7, 'arrived')):
  row(name, us(c[:, s] - t0))
h = sac[3][2 * parts * nt:2 * parts * nt + 4 * nt]
h = h[h[:, 7] >= t0]
if h.size:
  row('helpers: both critics of the tile seen', us(h[:, 2] - t0))
  row('helpers: done', us(h[:, 7] - t0))
  # the helpers' tail (profiles/tail_loads.txt): everything behind the wait for the critics; slot 3 (behind tile_bwd_dx, dz2 in LDS) only in builds that stamp it
  row('helpers: critics seen -> done', us(h[:, 7] - h[:, 2]))
  if (h[:, 3] >= h[:, 2]).all():
    row('helpers: critics seen -> dz2 done', us(h[:, 3] - h[:, 2]))
    row('helpers: dz2 done -> done', us(h[:, 7] - h[:, 3]))
