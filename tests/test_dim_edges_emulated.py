"""The bodies of tests/test_dim_edges_gpu.py - every kernel family against its oracle at the state / action widths of tests/golden/inputs.py EDGE_DIMS - on the host
emulation of the kernels (tests/host_emu), with the parametrisation the GPU module itself declares (its pytest.mark.parametrize marks are read, not restated) and the
GPU's bounds. What the emulator can say about a width: the indexing, the tile padding, the row layout, the arithmetic. Alignment and the memory system need the GPU."""
import itertools
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, 'golden')]
import test_kernels_host_emulation as E  # noqa: E402
import test_dim_edges_gpu as G  # noqa: E402


def _cases():
  out = []
  for name, fn in vars(G).items():
    if not name.startswith('test_') or not callable(fn): continue
    axes = []
    for m in getattr(fn, 'pytestmark', []):
      if m.name != 'parametrize': continue
      names = [n.strip() for n in m.args[0].split(',')]
      ids = m.kwargs.get('ids')
      axis = []
      for v in m.args[1]:
        given = getattr(v, 'id', None)
        values = getattr(v, 'values', None)
        if values is None: values = v if len(names) > 1 else (v,)
        label = given or (ids(values[0]) if callable(ids) else '-'.join(str(x) for x in values))
        axis.append((dict(zip(names, values)), label))
      axes.append(axis)
    for combo in itertools.product(*axes) if axes else [()]:
      kw = {}
      for part, _ in combo: kw.update(part)
      out.append(pytest.param(name, kw, id='-'.join([name[5:]] + [label for _, label in combo])))
  return out


@pytest.mark.parametrize('body,kw', _cases())
def test_dim_edge_bodies_on_the_emulated_kernels(monkeypatch, tmp_path, body, kw):
  fn = getattr(G, body)
  tgp = E._emulated_product(monkeypatch, streams=getattr(fn, 'streams', False))
  E._timed_path_modules(monkeypatch, tgp)
  for fixture, value in (('monkeypatch', monkeypatch), ('tmp_path', tmp_path)):
    if fixture in fn.__code__.co_varnames[:fn.__code__.co_argcount]: kw = dict(kw, **{fixture: value})
  fn(**kw)
