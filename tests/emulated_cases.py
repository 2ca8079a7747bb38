"""What the emulated runs of the `-m gpu` edge modules share (tests/test_dim_edges_emulated.py, tests/test_size_edges_emulated.py): the cases a GPU module declares,
read from its own pytest.mark.parametrize marks instead of being restated."""
import itertools

import pytest


def cases(module):
  out = []
  for name, fn in vars(module).items():
    if not name.startswith('test_') or not callable(fn) or getattr(fn, '__module__', None) != module.__name__: continue
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


def run(E, module, monkeypatch, tmp_path, body, kw):
  """One body of `module` on the emulated product (E = tests/test_kernels_host_emulation.py): streams and graphs only where the body asks for them (`fn.streams`)."""
  fn = getattr(module, body)
  tgp = E._emulated_product(monkeypatch, streams=getattr(fn, 'streams', False))
  E._timed_path_modules(monkeypatch, tgp)
  for fixture, value in (('monkeypatch', monkeypatch), ('tmp_path', tmp_path)):
    if fixture in fn.__code__.co_varnames[:fn.__code__.co_argcount]: kw = dict(kw, **{fixture: value})
  fn(**kw)
