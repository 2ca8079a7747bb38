"""An acting worker must not let go of a pinned mailbox that a queued launch still reads (imitation_learning_amd/acting.py `_drain`): torch's host allocator hands a freed
pinned block to the next pinned allocation at once, whose fill then rewrites the payload under the launch. tests/test_population_acting_gpu.py builds its per-learner
reference from temporaries (`_run_single(il.ActingWorker(...), ...)`) and now and then found part of a learner's last next_state zeroed by the next worker's mailbox."""
import numpy as np
import pytest

from imitation_learning_amd import acting


class _Box:
  o_echo = 3

  def __init__(self, word, echo):
    self.host, self.word, self.waited = np.array([word, 0, 0, echo], np.float32), word, []

  def wait(self, seq, what):
    self.waited.append((seq, what))


class _Block:
  def __init__(self, words):
    self.words, self.waited = words, []

  def wait(self, what):
    self.waited.append(what)


def test_a_dropped_worker_waits_for_the_echo_of_its_last_asynchronous_append():
  box = _Box(word=129.0, echo=65.0)           # the append's post has not been echoed yet
  acting._drain(box, True, 'append')
  assert box.waited == [(129.0, 'append')]
  for box, launched in ((_Box(129.0, 129.0), True), (_Box(129.0, 65.0), False), (_Box(0.0, -1.0), True)):   # echoed / posted without a launch (overlap schedule) / never posted
    acting._drain(box, launched, 'append')
    assert box.waited == []
  block = _Block(np.array([129.0, 130.0], np.float32))
  acting._drain(block, True, 'population append')
  assert block.waited == ['population append']
  for block, launched in ((_Block(None), True), (_Block(np.zeros(2, np.float32)), False)):
    acting._drain(block, launched, 'population append')
    assert block.waited == []
  acting._drain(None, True, 'a worker whose constructor raised')


def test_both_workers_drain_when_they_are_dropped():
  for cls in (acting.ActingWorker, acting.PopulationActingWorker):
    w = object.__new__(cls)
    w._append_box, w._append_launched = _Box(129.0, 65.0), True
    box = w._append_box
    del w
    assert box.waited and box.waited[0][0] == 129.0, cls.__name__


@pytest.mark.gpu
def test_a_freed_pinned_block_is_handed_to_the_next_allocation_at_once():
  """What `_drain` is for, shown on the allocator itself: a pinned tensor of a mailbox's size, dropped, gives its block to the next pinned allocation of that size - while
  a launch that was given the raw pointer could still be queued - and `torch.zeros(..., pin_memory=True)` fills it from the host straight away."""
  import torch
  n = 272
  a = torch.full((n,), 7.0).pin_memory()
  ptr = a.data_ptr()
  del a
  b = torch.zeros(n, dtype=torch.float32, pin_memory=True)
  assert b.data_ptr() == ptr and not b.any()
