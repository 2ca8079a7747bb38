"""Developer tool: the two legs of the forward / critic-loss launch and their join, as intervals, from a -DIL_TIMELINE build - the stamps of
pair_timeline.py, reported relative to each leg's own start instead of the index draw:

  bash profiles/tools/build_variants.sh tl:"-DIL_TIMELINE"
  IL_HIP_LIBRARY=variants/tl/libil_hip.so python profiles/tools/chain_legs_timeline.py [updates] [direct|graph]

min / median / max over the workgroups of a role, microseconds, of the LAST update. `direct` (default): back-to-back direct launches, the timed regime of bench.py."""
import ctypes as C
import sys
sys.path.insert(0, '.')
import numpy as np, torch, bench
from imitation_learning_amd import _lib

K, W, S = 12, 512, 8   # IL_TL_K, IL_TL_WGS, IL_TL_SLOTS (csrc/il_common.hpp)
plan, nets, _ = bench.build(torch.device('cuda', 0), 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
mode = sys.argv[2] if len(sys.argv) > 2 else 'direct'
if mode == 'direct':
  for _ in range(3): plan.run()
  torch.cuda.synchronize()
  plan.record_direct()
  for _ in range(n): plan.launch_direct(join=False)
  plan.join()
else:
  plan.capture(warmup=3)
  for _ in range(n): plan.replay()
torch.cuda.synchronize()
assert plan.sync_timeouts() == 0 and not plan.poisoned()
raw = C.CDLL(_lib.LIB_PATH)


def read(fn):
  buf = (C.c_ulonglong * (K * W * S))()
  assert getattr(raw, fn)(buf) == 0
  return np.frombuffer(buf, dtype=np.uint64).reshape(K, W, S).astype(np.int64)


sac, gail = read('il_debug_timeline_sac'), read('il_debug_timeline_gail')
B, nt = plan.B, plan.B // 16


def row(name, a):
  a = np.asarray(a, np.float64) / 100.0
  print(f'  {name:66s} {a.min():8.2f} {np.median(a):8.2f} {a.max():8.2f}   (n = {a.size})')


c = sac[10]
t_chain = c[:10 * nt, 0].min()   # the chain launch's first workgroup
print(f'B = {B}; {mode} launches, {n} updates; us; min / median / max over workgroups')
print("target leg: k_sac_chain_pair, after each workgroup's own start unless it says otherwise")
for lo, name in ((0, "actor(s') half 1"), (nt, "actor(s') half 0")):
  a = c[lo:lo + nt]
  row(f'{name}: prologue done', a[:, 1] - a[:, 0]); row(f'{name}: rows in LDS', a[:, 2] - a[:, 0]); row(f'{name}: layer 1 done', a[:, 3] - a[:, 0])
a = c[nt:2 * nt]; row("actor(s') half 0: arrival, after the launch's first workgroup", a[:, 7] - t_chain)
row("actor(s') half 0: partner's half received -> head done (slots 5 -> 6)", a[:, 6] - a[:, 5])   # (the head: profiles/tail_loads.txt)
a = c[2 * nt:6 * nt]; row("targets, both halves: a' seen -> layer 1 done (slots 2 -> 3)", a[:, 3] - a[:, 2])   # (the first layer in two parts)
a = c[4 * nt:6 * nt]; row("targets half 0: arrival, after the launch's first workgroup", a[:, 7] - t_chain)
a = c[6 * nt:7 * nt]; row("relabel: rewards written, after the launch's first workgroup", a[:, 6] - t_chain)
a = c[7 * nt:9 * nt]
row("critics: targets + rewards seen, after the launch's first workgroup", a[:, 5] - t_chain)
row('critics: targets + rewards seen -> done', a[:, 7] - a[:, 5])
row("critics: done, after the launch's first workgroup", a[:, 7] - t_chain)
row("k_sac_chain_pair: last stamp of any role, after the first workgroup", [c[:10 * nt + 3, 7].max() - t_chain])
print('reward leg: k_gail_grad (slot 2 = the wait that precedes the Philox counter: the epoch for the mixing call; on the parent for every call)')
kinds = [np.array([x + (nt + 1) * y for x in range(nt)]) for y in range(3)]
epoch = np.median(gail[0, kinds[2], 2])
for y, name in enumerate(('policy call', 'expert call', 'gradient-penalty call')):
  g = gail[0, kinds[y]]
  row(f'{name}: slot 2, relative to the gradient-penalty call seeing the epoch', g[:, 2] - epoch)
  row(f'{name}: rows staged (slot 4) after the epoch was seen', g[:, 4] - epoch)
  row(f'{name}: done after the epoch was seen', g[:, 7] - epoch)
row('k_gail_grad: last workgroup done after the epoch was seen', [max(gail[0, k, 7].max() for k in kinds) - epoch])
nr = int((gail[1, :, 7] >= epoch).sum())
row('k_gail_reduce: done after the epoch was seen', gail[1, :nr, 7] - epoch)
row("chain launch's first workgroup after the epoch was seen", [t_chain - epoch])
