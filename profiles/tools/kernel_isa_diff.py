#!/usr/bin/env python3
"""Compare the kernels of two sets of device assembly files (hipcc <Makefile CXXFLAGS> --cuda-device-only -S), kernel by kernel: the instruction text between a kernel's
label and its .Lfunc_end - comments, .loc-style directives and alignment padding removed, local labels renumbered in order of appearance - and its .amdhsa_ descriptor
block. A refactor that reports 0 differing kernels ships the same code. Usage: kernel_isa_diff.py OLD_DIR_OR_S NEW_DIR_OR_S (exit status 1 if anything differs)."""
import re, sys, hashlib, glob, os

def kernels(paths):
  out = {}
  for p in paths:
    txt = open(p).read().split('\n')
    names = [m.group(1) for l in txt for m in [re.match(r'\s*\.amdhsa_kernel (\S+)', l)] if m]
    for name in names:
      start = next(i for i, l in enumerate(txt) if l.startswith(name + ':'))
      end = next(i for i in range(start, len(txt)) if txt[i].startswith('.Lfunc_end'))
      body = []
      labels = {}
      for l in txt[start + 1:end]:
        l = re.sub(r';.*', '', l).strip()
        if not l or l.startswith(('.loc', '.file', '.cfi', '.p2align')): continue
        body.append(l)
      # renumber local labels in order of appearance
      def ren(m):
        return labels.setdefault(m.group(0), f'.L{len(labels)}')
      body = [re.sub(r'\.L[A-Za-z_]*\d+(_\d+)?', ren, l) for l in body]
      ds = next(i for i, l in enumerate(txt) if re.match(r'\s*\.amdhsa_kernel ' + re.escape(name) + r'\s*$', l))
      de = next(i for i in range(ds, len(txt)) if '.end_amdhsa_kernel' in txt[i])
      desc = [l.strip() for l in txt[ds:de]]
      out[name] = (body, desc)
  return out

a = kernels(sorted(glob.glob(os.path.join(sys.argv[1], '*.s'))) if os.path.isdir(sys.argv[1]) else [sys.argv[1]])
b = kernels(sorted(glob.glob(os.path.join(sys.argv[2], '*.s'))) if os.path.isdir(sys.argv[2]) else [sys.argv[2]])
bad = 0
for k in sorted(set(a) | set(b)):
  if k not in a or k not in b:
    print('ONLY IN', 'A' if k in a else 'B', k); bad += 1; continue
  same_body, same_desc = a[k][0] == b[k][0], a[k][1] == b[k][1]
  if not (same_body and same_desc):
    bad += 1
    print(f'DIFF {k}: body {"same" if same_body else f"differs ({len(a[k][0])} vs {len(b[k][0])} lines)"}, descriptor {"same" if same_desc else "differs"}')
    if not same_desc:
      for x, y in zip(a[k][1], b[k][1]):
        if x != y: print('   ', x, '->', y)
    for f in ('next_free_vgpr', 'next_free_sgpr', 'group_segment_fixed_size', 'private_segment_fixed_size'):   # VGPRs, SGPRs, LDS bytes, scratch bytes
      va, vb = [next(l.split()[-1] for l in d if '.amdhsa_' + f in l) for d in (a[k][1], b[k][1])]
      print(f'    {f}: {va} -> {vb}')
print(f'{len(a)} / {len(b)} kernels, {bad} differ')
sys.exit(1 if bad else 0)
