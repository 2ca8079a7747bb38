"""CPU: `+evaluation.schedule=lockstep` with general actor shapes - train.lockstep_evaluator's order (il.LockstepEvaluator first, il.GeneralLockstepEvaluator on its
refusal, the sequential schedule with ONE line when both refuse) with both classes replaced by stand-ins, and acting.general_lockstep_refusal clause by clause on stand-in
actors: the tile-engine predicate of il_actor_act_general (csrc/general.hip gt_env() && gt_shape_ok) restated from an actor's fields."""
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)

from imitation_learning_amd import config  # noqa: E402

LOCKSTEP = ['algorithm=SAC', 'reinforcement.actor.depth=3', 'reinforcement.actor.activation=tanh', '+evaluation.schedule=lockstep']


def _stand_ins(monkeypatch, fused, general):
  """Replaces both evaluator classes of train.il; each stand-in records (actors, max_rows) and returns or raises what `fused` / `general` (callables of the call index) say."""
  import train
  calls = {'fused': [], 'general': []}

  def make(name, behaviour):
    def cls(actors, max_rows):
      calls[name].append((list(actors), max_rows))
      return behaviour(len(calls[name]) - 1)
    return cls
  monkeypatch.setattr(train.il, 'LockstepEvaluator', make('fused', fused))
  monkeypatch.setattr(train.il, 'GeneralLockstepEvaluator', make('general', general))
  return train, calls


def _refuse(text):
  def behaviour(i): raise NotImplementedError(text)
  return behaviour


def test_the_fused_evaluator_accepts_and_the_general_one_is_never_built(monkeypatch, capsys):
  train, calls = _stand_ins(monkeypatch, lambda i: ('fused', i), lambda i: pytest.fail('the general evaluator was built although the fused one accepted'))
  cfg = config.compose(LOCKSTEP)
  a, b = object(), object()
  assert train.lockstep_evaluator(cfg, [a, b]) == ('fused', 0) and calls['fused'] == [([a, b], 30)]
  assert train.lockstep_evaluator(cfg, [a, b], each=True) == [('fused', 1), ('fused', 2)] and calls['fused'][1:] == [([a], 30), ([b], 30)]
  assert calls['general'] == [] and capsys.readouterr().err == ''


def test_the_fused_evaluator_refuses_and_the_general_one_is_returned_silently(monkeypatch, capsys):
  train, calls = _stand_ins(monkeypatch, _refuse('LockstepEvaluator: learner 0: an actor outside depth 2 / ReLU'), lambda i: ('general', i))
  cfg = config.compose(LOCKSTEP + ['evaluation.episodes=7'])
  a, b = object(), object()
  assert train.lockstep_evaluator(cfg, [a, b]) == ('general', 0)
  assert calls['fused'] == [([a, b], 7)] and calls['general'] == [([a, b], 7)]   # tried the same way: the same actors, the same rows
  assert train.lockstep_evaluator(cfg, [a, b], each=True) == [('general', 1), ('general', 2)] and calls['general'][1:] == [([a], 7), ([b], 7)]
  assert capsys.readouterr().err == ''


def test_both_refuse_one_line_with_both_reasons(monkeypatch, capsys):
  train, calls = _stand_ins(monkeypatch, _refuse('LockstepEvaluator: learner 0: an actor outside depth 2 / ReLU'), _refuse('GeneralLockstepEvaluator: learner 0: hidden 40 is not a multiple of 16'))
  cfg = config.compose(LOCKSTEP)
  assert train.lockstep_evaluator(cfg, [object()]) is None
  err = capsys.readouterr().err
  assert err.count('[train] evaluation:') == 1 and err.count('\n') == 1
  assert 'an actor outside depth 2 / ReLU' in err and 'hidden 40 is not a multiple of 16' in err and 'sequential' in err
  assert err.index('an actor outside depth 2') < err.index('hidden 40') < err.index('sequential')   # the first refusal's text as before, then the general evaluator's
  assert len(calls['fused']) == len(calls['general']) == 1


def test_per_learner_refusal_part_way_is_one_line_for_the_run(monkeypatch, capsys):
  """each=True over three learners: the fused evaluator refuses the first, the general one serves two and refuses the third - no evaluator for the run, one line."""
  def general(i):
    if i == 2: raise NotImplementedError('GeneralLockstepEvaluator: learner 0: state_size 600 is outside 1..512')
    return ('general', i)
  train, calls = _stand_ins(monkeypatch, _refuse('LockstepEvaluator: learner 0: no lockstep evaluation launch'), general)
  cfg = config.compose(LOCKSTEP)
  assert train.lockstep_evaluator(cfg, [object(), object(), object()], each=True) is None
  err = capsys.readouterr().err
  assert err.count('[train] evaluation:') == 1 and err.count('\n') == 1 and 'no lockstep evaluation launch' in err and 'state_size 600' in err
  assert len(calls['fused']) == 1 and len(calls['general']) == 3


def test_sequential_schedule_builds_neither(monkeypatch, capsys):
  train, calls = _stand_ins(monkeypatch, lambda i: pytest.fail('built'), lambda i: pytest.fail('built'))
  assert train.lockstep_evaluator(config.compose(['algorithm=SAC', 'reinforcement.actor.depth=3']), [object()]) is None
  assert capsys.readouterr().err == ''


def test_the_real_general_evaluator_refuses_a_plain_object_without_reading_it(monkeypatch, capsys):
  """The stand-in actors of tests/test_eval_schedule_config_cpu.py are plain object()s: the general evaluator's refusal is decided from the missing `general` attribute
  alone - nothing else is read and the library is not loaded."""
  import train
  from imitation_learning_amd import _lib, acting
  monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the library was loaded for an object that is no general actor'))

  class Fused:
    general = False
    def __getattr__(self, name): pytest.fail(f'{name} of a fused actor was read')

  for thing in (object(), Fused(), None, types.SimpleNamespace(general=0)):
    assert 'not a general-shape actor' in acting.general_lockstep_refusal(thing) and 'il_act_eval_rows' in acting.general_lockstep_refusal(thing, 30)
    with pytest.raises(NotImplementedError, match='GeneralLockstepEvaluator: learner 0: not a general-shape actor'):
      train.il.GeneralLockstepEvaluator([thing], 4)
  with pytest.raises(NotImplementedError, match='GeneralLockstepEvaluator: learner 0: not a general-shape actor'):
    train.il.GeneralLockstepEvaluator(object(), 4)   # one actor, not in a list


def _actor(**kw):
  fields = dict(general=True, hidden=48, depth=3, activation='tanh', state_size=17, action_size=6)
  fields.update(kw)
  return types.SimpleNamespace(**fields)


def test_general_lockstep_refusal_clause_by_clause(monkeypatch):
  from imitation_learning_amd.acting import general_lockstep_refusal as refusal
  monkeypatch.delenv('IL_GENERAL_TILES', raising=False)
  served = [_actor(), _actor(hidden=16, depth=1), _actor(hidden=512, depth=8, activation='sigmoid', state_size=512, action_size=8), _actor(hidden=96, depth=2, activation='relu'),
            _actor(state_size=1, action_size=1), _actor(hidden=256, depth=3, activation='relu')]
  for a in served:
    assert refusal(a) is None and refusal(a, 1024) is None, vars(a)
  for kw, words in ((dict(hidden=40), 'hidden 40 is not a multiple of 16'), (dict(hidden=528), 'hidden 528'), (dict(hidden=0), 'hidden 0'), (dict(hidden=8), 'hidden 8'),
                    (dict(hidden=1024), 'hidden 1024'), (dict(state_size=513), 'state_size 513 is outside 1..512'), (dict(state_size=0), 'state_size 0'),
                    (dict(action_size=9), 'action_size 9 is outside 1..8'), (dict(action_size=0), 'action_size 0'), (dict(depth=0), 'depth 0 is outside 1..8'),
                    (dict(depth=9), 'depth 9 is outside 1..8'), (dict(activation='gelu'), 'activation gelu')):
    assert words in refusal(_actor(**kw)), kw
  for bad in (0, 1025, -3):
    assert f'max_rows {bad} is outside 1..1024' in refusal(_actor(), bad)
  # IL_GENERAL_TILES as gt_env reads it: set, and its first character is `0`
  for value, off in (('0', True), ('0x', True), ('00', True), ('1', False), ('', False), ('10', False), ('off', False)):
    monkeypatch.setenv('IL_GENERAL_TILES', value)
    got = refusal(_actor())
    assert (got is not None and 'IL_GENERAL_TILES=0' in got) if off else got is None, value
  monkeypatch.setenv('IL_GENERAL_TILES', '0')
  assert 'hidden 40' in refusal(_actor(hidden=40))       # a shape clause is named ahead of the switch
  assert 'not a general-shape actor' in refusal(_actor(general=False))


def test_binding_and_exports():
  import ctypes as C
  import imitation_learning_amd as il
  from imitation_learning_amd import _lib, acting
  assert il.GeneralLockstepEvaluator is acting.GeneralLockstepEvaluator and issubclass(il.GeneralLockstepEvaluator, il.LockstepEvaluator)
  res, args = _lib._SIGNATURES['il_act_eval_rows_general']
  assert res is C.c_int and len(args) == len(_lib._SIGNATURES['il_act_eval_rows'][1]) + 2   # + depth, activation
  assert hasattr(C.CDLL(_lib.LIB_PATH), 'il_act_eval_rows_general')
  for hook in ('_refusal', '_shares_shape', '_call', '_entry'):   # the shared body: the general class replaces the hooks and nothing else
    assert hook in vars(acting.GeneralLockstepEvaluator) and hook in vars(acting.LockstepEvaluator)
  assert set(vars(acting.GeneralLockstepEvaluator)) - {'__module__', '__doc__', '__qualname__', '__firstlineno__', '__static_attributes__'} == {'_refusal', '_shares_shape', '_call', '_entry'}
