"""Acting worker: the per-environment-step part of the reference loop (train.py:151-168) with the device work of one step in one launch.

The reference does, per env step, `actor(state).sample()` (models.py:90-94), `memory.append(...)` (memory.py:40-44) and, when an
episode ends by true termination with absorbing=true, `memory.wrap_for_absorbing_states()` (memory.py:65-68).  Here those three are
`il_act_step`: the host writes the observation / reward / flags into a pinned, device-mapped mailbox, launches ONE kernel, and spins
on the sequence-number echo the kernel stores (system-scope release) after the action — no stream synchronisation, no H2D/D2H copies,
no per-field device ops.  The ring cursor is advanced on the device; the host mirrors it arithmetically for the index draws.

General actor shapes (any depth 1-8, relu / tanh / sigmoid, wide action spaces: `SoftActor.general`) take `il_act_step_general`: the same mailbox, carry and cursor, ONE launch
where the tile engine of csrc/general.hip applies (hidden a multiple of 16 up to 512, state <= 512, action <= 8), otherwise the per-function path's layer-at-a-time launches
reading the mailbox plus one commit kernel (still no copies or synchronisation; exact and fused schedules only - a snapshot read across several launches could tear).

Schedules:
  exact   : act(obs) -> env.step -> append(transition) -> [update]           (reference order; 2 launches, 1 wait per env step)
  fused   : step(transition, obs) = append + act in ONE launch on the update stream (the action of step t+1 is sampled before update t)
  overlap : `ActingWorker(..., mirror=True)`: act runs on its OWN stream against a published snapshot of the actor (il_act_publish, three
            slots + a version word), so the host gets its action in ~15 us and steps the environment WHILE the GPU runs the update;
            the append and the publish ride in the update's stream / hipGraph (UpdatePlan.pre_hooks / post_hooks). The behaviour
            policy lags the learner by one to two updates (what a host-side actor mirror would do).

Population (`PopulationActingWorker`): L learners of one fused actor shape (a seed sweep in one process) step in lockstep through `il_act_step_population` - ONE launch
of L workgroups and one wait for L echoes per act / append / step, instead of L launches and L turn-arounds. Every learner keeps its own mailbox, carry, ring, cursor,
Philox seed and offset; a learner with nothing to do in a launch idles (it gets its echo, nothing else of it is touched). With `reward_models` (one PWILDiscriminator
per learner) every launch that appends is preceded by ONE `il_pwil_act_reward_population` launch - the learner is a grid axis, so the L merges run side by side.

PWIL (`ActingWorker(..., reward_model=PWILDiscriminator)`): the reward of a transition is the greedy coupling of its (state, action) against the expert atoms
(models.py:216-249), which the per-function loop computes with a launch and a `.item()` per step. Here every launch that appends is preceded, on the same stream, by ONE
coupling launch (`il_pwil_act_reward`) that reads the pending transition where the append reads it, leaves the reward in the carry and - at an episode end - sets the
atom weights back itself: the reward never visits the host, and the caller issues no `reset()`.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import torch

from . import _lib

PENDING, WRAP_ABSORBING, GREEDY, NO_ACTION, CARRY_FROM_MAILBOX, REWARD_ON_DEVICE = 1, 2, 4, 8, 16, 32  # IL_ACT_* (include/il_hip.h)
_HEADER = 8
_NOISE_OFFSET = 6   # ACT_MAIL_NOISE_OFFSET (csrc/act_mail.hpp): il_act_step_population reads the learner's Philox offset here, as raw uint32 bits
_SEQ_MOD = 1 << 17  # the commit word (sequence * 64 + flags) travels as fp32: < 2^23


class _Mailbox:
  """Host view of one il_act_step mailbox (layout documented in include/il_hip.h)."""

  def __init__(self, S: int, A: int):
    n = int(_lib.lib().il_act_mailbox_floats(S, A))
    self.tensor = torch.zeros(n, dtype=torch.float32, pin_memory=True)
    self.host = self.tensor.numpy()
    Sp, Ap = (S + 3) & ~3, (A + 3) & ~3
    self.S, self.A = S, A
    self.o_next, self.o_obs, self.o_act = _HEADER, _HEADER + Sp, _HEADER + 2 * Sp
    self.o_echo = self.o_act + Ap
    assert self.o_echo < n
    self.word = 0.0          # commit word of the last post
    self.host[self.o_echo] = -1.0

  def post(self, seq: int, flags: int, reward: float = 0.0, terminal: float = 0.0, timeout: float = 0.0, step: float = 0.0, next_obs=None, obs=None, action=None) -> float:
    """Payload first, commit word (sequence * 64 + flags) last: a launch that is already queued sees either the previous post or this one, whole."""
    h = self.host
    h[2:6] = (reward, terminal, timeout, step)
    if next_obs is not None:
      h[self.o_next:self.o_next + self.S] = next_obs
    if obs is not None:
      h[self.o_obs:self.o_obs + self.S] = obs
    if action is not None:
      h[self.o_act:self.o_act + self.A] = action
    self.word = float(seq * 64 + flags)
    h[0] = self.word
    return self.word

  def wait(self, seq: float, what: str, timeout_s: float = 10.0):
    h, e = self.host, self.o_echo
    spins = 0
    while h[e] != seq:
      spins += 1
      if spins & 0xFFFF == 0:
        if time.perf_counter() - self._t0 > timeout_s:
          torch.cuda.synchronize()  # surfaces an asynchronous launch failure, if that is what happened
          raise RuntimeError(f'{what}: no echo from the device after {timeout_s:.0f} s (sequence {seq}, mailbox holds {h[e]})')
      elif spins == 1:
        self._t0 = time.perf_counter()


def _drain(box, launched: bool, what: str):
  """Before a worker lets go of its append mailbox: wait for the echo of the last post if a launch for it has been issued. The mailbox is pinned host memory that a queued
  launch reads through a raw pointer; once the tensor is freed torch's host allocator hands the block to the next pinned allocation of that size at once (it knows of no
  stream that uses it: tests/test_acting_mailbox_lifetime_cpu.py shows the reuse on the GPU), and that allocation's fill then rewrites the payload under the launch - a
  worker dropped right behind an asynchronous `append` lost part of its last next_state that way. The act mailbox needs no such wait: `act` and `step` return with its
  echo. Only `append` (the exact schedule) marks a launch: the overlap schedule's posts are consumed by `enqueue_append` launches that a plan may have captured or recorded
  (no echo comes until it replays them), and train.py keeps such a worker alive until the plan has been joined."""
  if box is None or not launched: return
  word = getattr(box, 'word', None)
  try:
    if word is None:                                                       # a _MailboxBlock: every learner's echo
      if getattr(box, 'words', None) is not None: box.wait(what)
    elif word and box.host[box.o_echo] != word: box.wait(word, what)
  except RuntimeError:   # no echo within the bound (a failed launch): nothing left to protect, and __del__ must not raise
    pass


def _row(x) -> np.ndarray:
  if torch.is_tensor(x):
    x = x.detach().to('cpu', torch.float32).numpy()
  return np.asarray(x, dtype=np.float32).reshape(-1)


def general_one_launch(actor) -> bool:
  """Whether il_act_step_general runs this general-shape actor's step as ONE launch (the tile engine of csrc/general.hip: hidden a multiple of 16 in 16..512, state <= 512,
  2 * action <= 16, IL_GENERAL_TILES != 0 - the predicate of il_actor_act_general) or as the layer-at-a-time launches plus a commit kernel (exact / fused schedules only)."""
  import os
  H = actor.hidden
  return (os.environ.get('IL_GENERAL_TILES', '1')[:1] != '0' and H % 16 == 0 and 16 <= H <= 512 and actor.state_size <= 512 and 2 * actor.action_size <= 16 and 1 <= actor.depth <= 8)


class ActingWorker:
  """One environment worker feeding one `ReplayMemory` from one `SoftActor` (train.py:151-168)."""

  def __init__(self, actor, memory, mirror: bool = False, reward_model=None, noise_seed=None):
    """`noise_seed`: the Philox seed of this worker's samples (default: torch.initial_seed()) - several workers in one process, one per learner of a sweep, take distinct ones."""
    assert _lib.on_device(actor.flat) and _lib.on_device(memory.ring), 'ActingWorker needs the actor and the ring on the GPU (there is no CPU path)'
    assert actor.state_size == memory.state_size and actor.action_size == memory.action_size
    self.general = bool(getattr(actor, 'general', False))
    self.one_launch = not self.general or general_one_launch(actor)
    if mirror and not self.one_launch:
      raise NotImplementedError(f'ActingWorker(mirror=True): the overlap schedule reads a parameter snapshot, which needs the one-launch acting step - hidden_size a multiple of 16 in 16..512, '
                                f'state_size <= 512, action_size <= 8 (IL_GENERAL_TILES != 0); this actor (state {actor.state_size}, action {actor.action_size}, hidden {actor.hidden}) acts through '
                                'several launches per step (csrc/general.hip): use the exact or the fused schedule')
    self.actor, self.memory = actor, memory
    self.S, self.A = memory.state_size, memory.action_size
    self.reward_model = reward_model   # a PWILDiscriminator: its coupling launch precedes every appending launch, and the append stores the reward that launch left in the carry
    if reward_model is not None:
      assert hasattr(reward_model, 'require_device_coupling'), 'ActingWorker(reward_model=...): a PWILDiscriminator (the one reward computed per environment step)'
      assert (reward_model.state_size, reward_model.action_size) == (self.S, self.A) and _lib.on_device(reward_model.expert_atoms)
      reward_model.require_device_coupling('ActingWorker(reward_model=...)')   # NotImplementedError outside the one-launch coupling's sizes
    self._reward_flag = REWARD_ON_DEVICE if reward_model is not None else 0
    self._act_box, self._append_box = _Mailbox(self.S, self.A), _Mailbox(self.S, self.A)
    dev = memory.ring.device
    self.carry = torch.zeros(self.S + self.A + 4, dtype=torch.float32, device=dev)
    self._seq = 0   # one sequence for both mailboxes: the device de-duplicates appends by commit word
    self._seed = C.c_uint64((torch.initial_seed() if noise_seed is None else int(noise_seed)) & (2**64 - 1))
    self._fixed = {}
    self._pending_seq = None
    self._workspace = None
    if self.general:   # il_act_step_general: depth, activation id and the per-function path's workspace at n = 1, kept with the worker
      from .models import ACTIVATION_IDS
      self._depth, self._activation = actor.depth, ACTIVATION_IDS[actor.activation]
      need = int(_lib.lib().il_actor_workspace_floats_general(self.S, self.A, actor.hidden, actor.depth, 1))
      self._workspace = torch.zeros(need, dtype=torch.float32, device=dev)
    self.mirror = None
    if mirror:
      self._stride = (actor.flat.numel() + 63) // 64 * 64
      self.mirror = torch.zeros(3, self._stride, dtype=torch.float32, device=dev)
      self._version = torch.zeros(2, dtype=torch.int32, device=dev)   # {snapshot version, completion counter of k_act_publish}
      self.act_stream = torch.cuda.Stream(device=dev, priority=-1)     # short, latency-critical launches next to the update graph
      self.enqueue_publish()
      torch.cuda.current_stream().synchronize()

  def _launch(self, box: _Mailbox, acts: bool = True, stream=None, snapshot: bool = False, appends: bool = False):
    """`appends`: the launch may find a pending transition in `box` - with a reward model its coupling launch goes first (library call, fixed pointers: recordable)."""
    a = self.actor
    a._act_calls += int(acts)  # the Philox offset is shared with SoftActor._act, so the two entry points never reuse noise
    key = (id(box), snapshot)
    fixed = self._fixed.get(key)
    if fixed is None or fixed[0] != a.flat.data_ptr():  # pointers are stable for the life of the worker; re-derive if the arena was re-homed
      params = self.mirror if snapshot else a.flat
      fixed = self._fixed[key] = (a.flat.data_ptr(), None, _lib.ptr(params), C.c_void_p(box.tensor.data_ptr()), _lib.ptr(self.carry),
                                  _lib.ptr(self.memory.ring), _lib.ptr(self.memory._ring_state), _lib.ptr(self._version) if snapshot else None,
                                  self._stride if snapshot else 0)
    _, _, p_actor, p_box, p_carry, p_ring, p_state, p_version, stride = fixed
    L = _lib.lib()   # (looked up per call: UpdatePlan.record_direct walks the hooks with a recording stand-in for the library)
    st = (stream or torch.cuda.current_stream()).cuda_stream
    if appends and self.reward_model is not None:
      rc = L.il_pwil_act_reward(C.byref(self.reward_model._desc), p_box, p_carry, st)   # (the descriptor lives with the discriminator, which this worker keeps alive)
      if rc: _lib.check(rc)
    if self.general:
      rc = L.il_act_step_general(p_actor, self.S, self.A, a.hidden, self._depth, self._activation, p_box, p_carry, p_ring, p_state, self._seed, a._act_calls & 0xFFFFFFFF, p_version, stride,
                                 _lib.ptr(self._workspace), self._workspace.numel(), st)
    else:
      rc = L.il_act_step(p_actor, self.S, self.A, a.hidden, p_box, p_carry, p_ring, p_state, self._seed, a._act_calls & 0xFFFFFFFF, p_version, stride, st)
    if rc: _lib.check(rc)

  def _next_seq(self) -> int:
    self._seq = self._seq % (_SEQ_MOD - 1) + 1   # 1 .. 2^17-1: never 0, so a zeroed carry matches nothing
    return self._seq

  def _collect(self, box: _Mailbox, seq: float) -> torch.Tensor:
    box.wait(seq, 'il_act_step')
    return torch.from_numpy(box.host[box.o_act:box.o_act + self.A].copy()).unsqueeze(0)

  def _mirror_append(self, terminal: bool, timeout: bool, wrap: bool):
    m = self.memory
    m._advance(terminal, timeout)
    if wrap:
      m._advance(False, False)

  # --- exact schedule (and the act half of the overlap schedule)
  def act(self, obs, greedy: bool = False) -> torch.Tensor:
    """`actor(obs).sample()` (or the greedy action) as a [1, A] CPU tensor. Without a mirror: on the current stream with the live
    parameters, remembering (obs, action) on the device for `append`. With a mirror: on the worker's own stream from the latest snapshot."""
    box = self._act_box
    seq = box.post(self._next_seq(), GREEDY if greedy else 0, obs=_row(obs))
    if self.mirror is None:
      self._launch(box)
    else:
      self._launch(box, stream=self.act_stream, snapshot=True)
    return self._collect(box, seq)

  def act_begin(self, obs, greedy: bool = False):
    """The launch half of `act` (round 6): post the observation and enqueue the act launch, return at once; `act_end()` collects the action. With a mirror the launch runs
    on the worker's own stream from the latest snapshot, so a caller can put its update's host work (a graph replay or the direct launches: ~30 us) between the two calls -
    the act launch's ~29 us turn-around (dispatch, one workgroup through the actor, the echo into pinned memory) then hides behind it instead of following it
    (profiles/r06_acting_host_profile.json: 96 -> us per environment step with one update per step)."""
    box = self._act_box
    self._pending_seq = box.post(self._next_seq(), GREEDY if greedy else 0, obs=_row(obs))
    if self.mirror is None:
      self._launch(box)
    else:
      self._launch(box, stream=self.act_stream, snapshot=True)

  def act_end(self) -> torch.Tensor:
    seq, self._pending_seq = self._pending_seq, None
    assert seq is not None, 'act_end() without act_begin()'
    return self._collect(self._act_box, seq)

  def append(self, step, next_obs, reward, terminal: bool, timeout: bool):
    """`memory.append(step, state, action, reward, next_state, terminal, timeout)` for the (state, action) of the last `act`, plus the
    absorbing wrap when the episode ended by true termination (train.py:157,161). Asynchronous: nothing is waited for.
    With a reward model the ring's reward is the device's (`reward` is the caller's, e.g. for its train_return), here and in `step` / `post`."""
    assert self.mirror is None, 'with a mirror the act launches run ahead of the appends: use post() + enqueue_append()'
    wrap = bool(self.memory.absorbing and terminal and not timeout)
    box = self._append_box
    if box.word: box.wait(box.word, 'il_act_step(append)')  # normally already echoed: the act in between ran after it on the same stream
    box.post(self._next_seq(), PENDING | NO_ACTION | self._reward_flag | (WRAP_ABSORBING if wrap else 0), float(reward), float(terminal), float(timeout), float(step), next_obs=_row(next_obs))
    self._launch(box, acts=False, appends=True)
    self._append_launched = True
    self._mirror_append(bool(terminal), bool(timeout), wrap)

  def __del__(self):
    _drain(getattr(self, '_append_box', None), getattr(self, '_append_launched', False), 'il_act_step(append)')

  # --- fused schedule
  def step(self, step, next_obs, reward, terminal: bool, timeout: bool, obs=None, greedy: bool = False) -> torch.Tensor:
    """append(transition of the last action) + act(obs) in ONE launch. `obs` defaults to `next_obs`; pass the reset observation when
    the episode ended."""
    assert self.mirror is None
    wrap = bool(self.memory.absorbing and terminal and not timeout)
    box = self._act_box
    nxt = _row(next_obs)
    seq = box.post(self._next_seq(), PENDING | self._reward_flag | (WRAP_ABSORBING if wrap else 0) | (GREEDY if greedy else 0), float(reward), float(terminal), float(timeout), float(step),
                   next_obs=nxt, obs=nxt if obs is None else _row(obs))
    self._launch(box, appends=True)
    self._mirror_append(bool(terminal), bool(timeout), wrap)
    return self._collect(box, seq)

  # --- overlap schedule: the append and the publish ride in the update stream (UpdatePlan.pre_hooks / post_hooks), the act runs beside it
  def post(self, step, obs, action, next_obs, reward, terminal: bool, timeout: bool):
    """Host side of an append: fill the append mailbox with the whole transition. The next `enqueue_append` launch (direct, or the one
    captured in an update graph) consumes it exactly once. Blocks only if the previous post has not been consumed yet (back-pressure:
    the host can run at most one update ahead of the GPU)."""
    box = self._append_box
    if box.word: box.wait(box.word, 'il_act_step(append)', timeout_s=30.0)
    wrap = bool(self.memory.absorbing and terminal and not timeout)
    box.post(self._next_seq(), PENDING | NO_ACTION | CARRY_FROM_MAILBOX | self._reward_flag | (WRAP_ABSORBING if wrap else 0), float(reward), float(terminal), float(timeout), float(step), next_obs=_row(next_obs),
             obs=_row(obs), action=_row(action))
    self._mirror_append(bool(terminal), bool(timeout), wrap)

  def enqueue_append(self):
    """Launch the append kernel on the current stream (capturable: every argument is a fixed pointer; what to append is read from the mailbox)."""
    self._launch(self._append_box, acts=False, appends=True)

  def enqueue_publish(self):
    """Snapshot the actor arena for the act stream; enqueue after anything that changes the actor (capturable)."""
    a = self.actor
    _lib.check(_lib.lib().il_act_publish(_lib.ptr(a.flat), a.flat.numel(), _lib.ptr(self.mirror), self._stride, _lib.ptr(self._version), _lib.stream_ptr()))

  enqueue_append._il_recordable = True    # UpdatePlan.record_direct: library calls only, every argument a fixed pointer (what to append / publish is read on the device)
  enqueue_publish._il_recordable = True

  def attach(self, plan):
    """Make `plan` (UpdatePlan) carry this worker's append before, and its parameter snapshot after, every update. Attach before capture."""
    assert self.mirror is not None and plan.graph is None
    plan.pre_hooks.append(self.enqueue_append)
    plan.post_hooks.append(self.enqueue_publish)
    return self


class _MailboxBlock:
  """Host view of L il_act_step mailboxes as ONE pinned [L, floats] block: a post is a few vectorised numpy writes, payload first, the L commit words last."""

  def __init__(self, L: int, S: int, A: int):
    n = int(_lib.lib().il_act_mailbox_floats(S, A))
    self.tensor = torch.zeros(L, n, dtype=torch.float32, pin_memory=True)
    self.host = self.tensor.numpy()
    self.bits = self.host.view(np.uint32)
    Sp, Ap = (S + 3) & ~3, (A + 3) & ~3
    self.L, self.S, self.A, self.floats = L, S, A, n
    self.o_next, self.o_obs, self.o_act = _HEADER, _HEADER + Sp, _HEADER + 2 * Sp
    self.o_echo = self.o_act + Ap
    assert self.o_echo < n
    self.host[:, self.o_echo] = -1.0
    self.echo = self.host[:, self.o_echo]
    self.words = None   # commit words of the last post

  def commit(self, seq: int, flags: np.ndarray) -> np.ndarray:
    self.words = (seq * 64 + flags).astype(np.float32)
    self.host[:, 0] = self.words
    return self.words

  def wait(self, what: str, timeout_s: float = 10.0):
    words, spins, t0 = self.words, 0, 0.0
    while not np.array_equal(self.echo, words):   # (self.echo: a view of the echo column here, a fresh gather of the per-learner slots in _MixedMailboxBlock)
      spins += 1
      if spins == 1:
        t0 = time.perf_counter()
      elif spins & 0xFFF == 0 and time.perf_counter() - t0 > timeout_s:
        torch.cuda.synchronize()  # surfaces an asynchronous launch failure, if that is what happened
        echo = self.echo
        missing = [l for l in range(self.L) if echo[l] != words[l]]
        raise RuntimeError(f'{what}: no echo from the device after {timeout_s:.0f} s for learner(s) {missing} (commit words {words[missing].tolist()}, mailboxes hold {echo[missing].tolist()})')


class _MixedMailboxBlock(_MailboxBlock):
  """L mailboxes of learners with different (S, A) as one pinned [L, widest mailbox] block: row l starts learner l's mailbox, laid out inside as
  il_act_mailbox_floats(S_l, A_l) lays it out, so the observation, action and echo slots sit at per-learner offsets (`o_obs`, `o_act`, `o_echo`: arrays)."""

  def __init__(self, L: int, Ss, As):
    assert len(Ss) == L and len(As) == L
    n = max(int(_lib.lib().il_act_mailbox_floats(S, A)) for S, A in zip(Ss, As))
    self.tensor = torch.zeros(L, n, dtype=torch.float32, pin_memory=True)
    self.host = self.tensor.numpy()
    self.bits = self.host.view(np.uint32)
    Sp, Ap = (np.asarray(Ss) + 3) & ~3, (np.asarray(As) + 3) & ~3
    self.L, self.S, self.A, self.floats = L, list(Ss), list(As), n
    self.o_next, self.o_obs, self.o_act = _HEADER, _HEADER + Sp, _HEADER + 2 * Sp
    self.o_echo = self.o_act + Ap
    assert int(self.o_echo.max()) < n
    self._ar = np.arange(L)
    self.host[self._ar, self.o_echo] = -1.0
    self.words = None

  @property
  def echo(self) -> np.ndarray:
    return self.host[self._ar, self.o_echo]   # a fresh read of every learner's echo slot


def _rows(xs, rows, width: int) -> np.ndarray:
  return np.stack([_row(xs[l])[:width] for l in rows])


def lockstep_refusal(actor, max_rows: int = 1):
  """None when `il_act_eval_rows` serves this actor; otherwise the predicate it misses, in words (LockstepEvaluator raises it, train.py prints it and evaluates
  sequentially). A fused-shape actor (`not actor.general`: depth 2, ReLU, hidden a multiple of 64 in 64..256, 2 * action_size <= 16) is inside the entry point's limits on
  hidden and action width by construction; what is left to ask here, because the evaluator sizes its pinned block from them before the first launch, is the state width
  against the workgroup and max_rows. The entry point itself checks all of them again on every launch (csrc/sac.hip il_act_eval_rows)."""
  if getattr(actor, 'general', False):
    return (f'an actor outside depth 2 / ReLU / hidden 64..256 in multiples of 64 / action_size <= 8 (depth {getattr(actor, "depth", "?")}, {getattr(actor, "activation", "?")}, hidden '
            f'{actor.hidden}, action_size {actor.action_size}) has no lockstep evaluation launch (general shapes are out of its scope)')
  H, S = actor.hidden, actor.state_size
  if S < 1 or 64 + S > max(256, 4 * H): return f'state_size {S} is outside 1 <= state_size and 64 + state_size <= {max(256, 4 * H)} (the workgroup at hidden {H})'
  if not 1 <= max_rows <= 1024: return f'max_rows {max_rows} is outside 1..1024'
  return None


def general_lockstep_refusal(actor, max_rows: int = 1):
  """None when `il_act_eval_rows_general` serves this actor; otherwise the predicate it misses, in words (GeneralLockstepEvaluator raises it, train.py prints it and
  evaluates sequentially). An object that is not a general-shape actor (`general` not true: a fused actor, or anything without the attribute) gets a reason and nothing
  else of it is read. For a general actor this restates the tile-engine predicate of il_actor_act_general (csrc/general.hip gt_env() && gt_shape_ok) from the actor's
  fields - the entry point has no layer-at-a-time form - with IL_GENERAL_TILES read as gt_env reads it: set, and its first character is `0`. The entry point itself checks
  all of it again on every launch."""
  import os
  if not getattr(actor, 'general', False):
    return 'not a general-shape actor (the fused shape - depth 2 / ReLU / hidden 64..256 in multiples of 64 - is served by il_act_eval_rows: LockstepEvaluator)'
  from .models import ACTIVATION_IDS
  H, S, A, depth = actor.hidden, actor.state_size, actor.action_size, actor.depth
  if not 1 <= depth <= 8: return f'depth {depth} is outside 1..8'
  if actor.activation not in ACTIVATION_IDS: return f'activation {actor.activation} is none of {sorted(ACTIVATION_IDS)}'
  if H % 16 != 0 or not 16 <= H <= 512:
    return f'hidden {H} is not a multiple of 16 in 16..512 (the one-launch tile engine; il_act_eval_rows_general has no layer-at-a-time form)'
  if not 1 <= S <= 512: return f'state_size {S} is outside 1..512 (the one-launch tile engine; il_act_eval_rows_general has no layer-at-a-time form)'
  if not 1 <= A <= 8: return f'action_size {A} is outside 1..8 (the one-launch tile engine; il_act_eval_rows_general has no layer-at-a-time form)'
  if os.environ.get('IL_GENERAL_TILES', '')[:1] == '0': return 'IL_GENERAL_TILES=0 switches the tile engine off (il_act_eval_rows_general has no layer-at-a-time form)'
  if not 1 <= max_rows <= 1024: return f'max_rows {max_rows} is outside 1..1024'
  return None


class LockstepEvaluator:
  """The greedy actions of up to `max_rows` observations per learner - one row per evaluation episode still running - in ONE `il_act_eval_rows` launch per lockstep step,
  for one `SoftActor` or several (one hidden size; their state / action widths may differ). Owns the mailboxes (one pinned block, learner l's laid out as
  il_eval_mailbox_floats(S_l, A_l, max_rows) lays it out) and the descriptor array on the device. Fused actor shapes only: a general shape raises NotImplementedError naming
  the predicate (`lockstep_refusal`). The launch reads live parameters and changes nothing on the device; nothing of the acting workers is touched.

  Pinned-memory lifetime (the rule of `_drain`): `act` returns with the echoes of the tiles that hold live rows; the tiles without one only echo, and may do so a little
  later. The next `act` waits for those before it posts (so a launch only ever sees its own post), and the evaluator waits for them before it lets go of the block.

  `GeneralLockstepEvaluator` is this class with three hooks replaced: the refusal predicate, what the learners have to share, and the library call."""

  _entry = 'il_act_eval_rows'

  def _refusal(self, actor, max_rows: int):
    return lockstep_refusal(actor, max_rows)

  def _shares_shape(self, a, a0):
    assert a.hidden == a0.hidden, f'LockstepEvaluator: one hidden size for all learners (got {a0.hidden} and {a.hidden})'

  def _call(self, lib, stream):
    return lib.il_act_eval_rows(_lib.ptr(self._descs), C.cast(self._descs_host, C.c_void_p), self.L, self.max_rows, self.H, stream)

  def __init__(self, actors, max_rows: int):
    actors = list(actors) if isinstance(actors, (list, tuple)) else [actors]
    max_rows = int(max_rows)
    who = type(self).__name__
    assert len(actors) >= 1, f'{who}: at least one actor'
    a0 = actors[0]
    for l, a in enumerate(actors):
      reason = self._refusal(a, max_rows)
      if reason is not None: raise NotImplementedError(f'{who}: learner {l}: {reason}')
      assert _lib.on_device(a.flat), f'{who} needs the actors on the GPU (there is no CPU path)'
      self._shares_shape(a, a0)
      assert a.flat.device == a0.flat.device
    from .training import _device_array
    lib = _lib.lib()
    L = len(actors)
    self.actors, self.L, self.H, self.max_rows, self.device = actors, L, a0.hidden, max_rows, a0.flat.device
    self.widths = [(int(a.state_size), int(a.action_size)) for a in actors]
    self.tiles = (max_rows + 15) // 16
    self.floats = max(int(lib.il_eval_mailbox_floats(S, A, max_rows)) for S, A in self.widths)
    self.tensor = torch.zeros(L, self.floats, dtype=torch.float32, pin_memory=True)
    self.host = self.tensor.numpy()
    self._flat = self.host.reshape(-1)
    self._obs, self._act, echo = [], [], []
    for l, (S, A) in enumerate(self.widths):
      Sp, Ap = (S + 3) & ~3, (A + 3) & ~3
      o_obs, o_act = _HEADER, _HEADER + max_rows * Sp
      o_echo = o_act + max_rows * Ap
      assert o_echo + self.tiles <= int(lib.il_eval_mailbox_floats(S, A, max_rows)) <= self.floats
      self._obs.append(self.host[l, o_obs:o_act].reshape(max_rows, Sp)[:, :S])   # views into the block
      self._act.append(self.host[l, o_act:o_echo].reshape(max_rows, Ap)[:, :A])
      echo.append(l * self.floats + o_echo + np.arange(self.tiles))
    self._echo = np.stack(echo)                      # [L, tiles] positions of the echo words in the block
    self._flat[self._echo.reshape(-1)] = -1.0
    base, stride = self.tensor.data_ptr(), self.floats * 4
    descs = [_lib.EvalLearner(a.flat.data_ptr(), base + l * stride, S, A) for l, (a, (S, A)) in enumerate(zip(actors, self.widths))]
    self._descs_host = (_lib.EvalLearner * L)(*descs)   # the entry point sizes the launch, and decides its refusals, on this copy
    self._descs = _device_array(descs, self.device)
    self._arenas = [a.flat.data_ptr() for a in actors]
    self._seq, self.word = 0, None   # word: the commit word of the last post
    self._in_flight = False          # a launch has been issued whose echoes (all tiles) have not all been seen yet

  def _next_seq(self) -> int:
    self._seq = self._seq % (_SEQ_MOD - 1) + 1   # ActingWorker._next_seq's rule: 1 .. 2^17-1, never 0
    return self._seq

  def _wait(self, where: np.ndarray, what: str, timeout_s: float = 10.0):
    flat, word, spins, t0 = self._flat, self.word, 0, 0.0
    while not (flat[where] == word).all():
      spins += 1
      if spins == 1:
        t0 = time.perf_counter()
      elif spins & 0xFFF == 0 and time.perf_counter() - t0 > timeout_s:
        torch.cuda.synchronize()  # surfaces an asynchronous launch failure, if that is what happened
        raise RuntimeError(f'{what}: no echo from the device after {timeout_s:.0f} s (commit word {word}, echoes hold {flat[where].tolist()})')

  def wait(self, what: str = None):
    """Every tile's echo of the last launched post, those without a live row included: behind it no workgroup of that launch reads or writes the block any more. Nothing
    to wait for when no launch is outstanding (a post that was never launched, or whose launch the entry point refused)."""
    if not self._in_flight: return
    self._wait(self._echo.reshape(-1), what or self._entry)
    self._in_flight = False

  def post(self, obs_per_learner) -> list:
    """Pack learner l's observations into rows [0, n_l) of its mailbox, then the row counts, then - last - the L commit words. Returns the row counts."""
    assert len(obs_per_learner) == self.L, f'{type(self).__name__}: one entry per learner ({self.L}), got {len(obs_per_learner)}'
    self.wait()
    counts = []
    for l, rows in enumerate(obs_per_learner):
      n = 0 if rows is None else len(rows)
      assert n <= self.max_rows, f'{type(self).__name__}: learner {l} has {n} rows, the mailbox holds {self.max_rows}'
      if n:
        S = self.widths[l][0]
        if torch.is_tensor(rows): rows = rows.detach().to('cpu', torch.float32).numpy()
        self._obs[l][:n] = rows.reshape(n, -1)[:, :S] if isinstance(rows, np.ndarray) else np.stack([_row(x)[:S] for x in rows])
      counts.append(n)
    self.host[:, 1] = counts
    self.word = np.float32(self._next_seq() * 64 + GREEDY)
    self.host[:, 0] = self.word
    return counts

  def launch(self):
    """ONE il_act_eval_rows (il_act_eval_rows_general) on the current stream (what to act on is read from the mailboxes)."""
    if any(a.flat.data_ptr() != p for a, p in zip(self.actors, self._arenas)):   # an arena was re-homed: re-derive the descriptors
      from .training import _device_array
      for l, a in enumerate(self.actors): self._descs_host[l].actor = a.flat.data_ptr()
      self._descs, self._arenas = _device_array(list(self._descs_host), self.device), [a.flat.data_ptr() for a in self.actors]
    rc = self._call(_lib.lib(), torch.cuda.current_stream().cuda_stream)
    if rc: _lib.check(rc)
    self._in_flight = True

  def act(self, obs_per_learner) -> list:
    """`obs_per_learner[l]`: the observations of learner l's still-running episodes (a list of rows or an [n_l, S_l] array; empty or None: the learner idles). Returns, per
    learner, the greedy actions as a CPU tensor [n_l, A_l]. Each actor's `_act_calls` advances by its n_l, as n_l `get_greedy_action` calls would have advanced it."""
    counts = self.post(obs_per_learner)
    self.launch()
    live = [self._echo[l, :(n + 15) // 16] for l, n in enumerate(counts) if n]
    if live: self._wait(np.concatenate(live), self._entry)
    out = []
    for l, n in enumerate(counts):
      self.actors[l]._act_calls += n
      out.append(torch.from_numpy(self._act[l][:n].copy()))
    return out

  def __del__(self):
    if getattr(self, '_in_flight', False):
      try: self.wait()
      except RuntimeError: pass   # no echo within the bound (a failed launch): nothing left to protect, and __del__ must not raise


class GeneralLockstepEvaluator(LockstepEvaluator):
  """`LockstepEvaluator` for general actor shapes: ONE `il_act_eval_rows_general` launch per lockstep step (csrc/general.hip k_act_eval_rows_general: the tile engine's
  forward on every 16-row tile). The same mailboxes, posts, waits and pinned-memory rules; per row the action is `get_greedy_action`'s (il_actor_act_general, greedy), bit
  for bit. Serves the shapes that entry point runs as one launch (`general_lockstep_refusal`); the learners share one (hidden, depth, activation), their state / action
  widths may differ. A fused-shape actor, a shape outside the tile engine and learners of different shapes raise NotImplementedError with the reason."""

  _entry = 'il_act_eval_rows_general'

  def _refusal(self, actor, max_rows: int):
    return general_lockstep_refusal(actor, max_rows)

  def _shares_shape(self, a, a0):
    mine, first = (a.hidden, a.depth, a.activation), (a0.hidden, a0.depth, a0.activation)
    if mine != first:
      raise NotImplementedError(f'GeneralLockstepEvaluator: one (hidden, depth, activation) for all learners of a launch (got {first} and {mine})')

  def _call(self, lib, stream):
    from .models import ACTIVATION_IDS
    a0 = self.actors[0]
    return lib.il_act_eval_rows_general(_lib.ptr(self._descs), C.cast(self._descs_host, C.c_void_p), self.L, self.max_rows, self.H, a0.depth, ACTIVATION_IDS[a0.activation], stream)


class PopulationActingWorker:
  """L environment workers - L `SoftActor`s of one hidden size feeding L `ReplayMemory`s - whose device work per lockstep environment step is ONE launch
  (`il_act_step_population`: workgroup l = learner l's `il_act_step`; learners of different state / action widths: `il_act_step_population_mixed`, mailboxes and carries
  laid out per learner, `act` / `step` / `act_eval` then return [L, widest A] with learner l's `widths[l][1]` components in row l and zeros behind them). `act` / `append` / `step` are `ActingWorker`'s exact and fused schedules over lists (entry l belongs to
  learner l); a `None` entry makes that learner idle in the launch. Every learner's `actor._act_calls`, `memory.idx / full / num_trajectories`, ring and cursor end up
  where its own `ActingWorker(actor, memory, noise_seed=noise_seeds[l])` would have left them. Fused actor shapes only (depth 2, ReLU, hidden 64..256 in multiples of 64);
  no mirror / overlap schedule. `reward_models`: None, or one PWILDiscriminator per learner (each on its own atoms: the learners of a sweep subsample their expert data
  under their own seeds) - `append` and `step` then post IL_ACT_REWARD_ON_DEVICE for every pending learner and enqueue `il_pwil_act_reward_population` directly ahead of
  the acting launch; the `reward` argument never reaches the ring, and no `reset()` is issued at episode ends (the kernel does it), as in `ActingWorker(reward_model=...)`."""

  def __init__(self, actors, memories, noise_seeds, reward_models=None):
    actors, memories, noise_seeds = list(actors), list(memories), [int(s) for s in noise_seeds]
    L = len(actors)
    if reward_models is not None:
      reward_models = list(reward_models) if isinstance(reward_models, (list, tuple)) else [reward_models]
      if all(r is None for r in reward_models): reward_models = None
    if reward_models is not None:
      if any(r is None for r in reward_models) or len(reward_models) != L:
        raise ValueError(f'PopulationActingWorker(reward_models=...): None, or one PWILDiscriminator per learner ({L}) - a list that mixes None with discriminators, or of another length, is refused')
      if not all(hasattr(r, 'require_device_coupling') for r in reward_models):
        raise NotImplementedError('PopulationActingWorker(reward_models=...): a PWIL reward model (PWILDiscriminator: the one reward computed per environment step, by il_pwil_act_reward_population) per learner')
    assert L >= 1 and len(memories) == L and len(noise_seeds) == L, 'PopulationActingWorker: one memory and one noise seed per actor'
    a0, m0 = actors[0], memories[0]
    if any(getattr(a, 'general', False) for a in actors):
      raise NotImplementedError('PopulationActingWorker: actor shapes outside depth 2 / ReLU / hidden 64..256 in multiples of 64 / action_size <= 8 have no population launch (one ActingWorker per learner)')
    for a, m in zip(actors, memories):
      assert _lib.on_device(a.flat) and _lib.on_device(m.ring), 'PopulationActingWorker needs the actors and the rings on the GPU (there is no CPU path)'
      assert (a.state_size, a.action_size) == (m.state_size, m.action_size), f'PopulationActingWorker: an actor of widths {(a.state_size, a.action_size)} feeds a memory of widths {(m.state_size, m.action_size)}'
      assert a.hidden == a0.hidden, f'PopulationActingWorker: one hidden size for all learners (got {a0.hidden} and {a.hidden})'
      assert m.ring.device == m0.ring.device and a.flat.device == a0.flat.device
    self.actors, self.memories, self.L = actors, memories, L
    self.S, self.A, self.H = m0.state_size, m0.action_size, a0.hidden
    self.device = m0.ring.device
    self._seeds = noise_seeds
    # learners of different (S, A) - the four environments of train_all.py - step through il_act_step_population_mixed: mailboxes and carries laid out per learner
    self.widths = [(int(m.state_size), int(m.action_size)) for m in memories]
    self.mixed = len(set(self.widths)) > 1
    self._dims = self._dims_host = None
    if self.mixed:
      if reward_models is not None:
        raise NotImplementedError('PopulationActingWorker(reward_models=...): learners of different state / action widths have no population coupling launch (one shape for all learners)')
      T = max(256, 4 * self.H)   # il_act_step's workgroup: the limits below are ITS limits, for each learner's own widths
      for l, (S, A) in enumerate(self.widths):
        row = int(_lib.lib().il_ring_row_floats(S, A))
        assert 2 * A <= 16 and row <= T and 64 + S <= T, f'PopulationActingWorker: learner {l} (state {S}, action {A}) is outside il_act_step\'s limits at hidden {self.H} (2A <= 16, ring row {row} and 64 + S within {T} threads)'
        assert memories[l].row == row, f'PopulationActingWorker: learner {l}: the memory\'s ring row ({memories[l].row} floats) is not il_ring_row_floats({S}, {A}) = {row}'
      from .training import _device_array
      dims = [_lib.ActDims(S, A, int(_lib.lib().il_ring_row_floats(S, A)), 0) for S, A in self.widths]
      self._dims_host = (_lib.ActDims * L)(*dims)   # the entry point sizes the launch, and decides its refusals, on this copy
      self._dims = _device_array(dims, self.device)
      self.S, self.A = [w[0] for w in self.widths], max(w[1] for w in self.widths)   # per-learner state widths; the action tensor is [L, widest A]
    cw = max(S + A for S, A in self.widths) + 4
    self.carry = torch.zeros(L, cw, dtype=torch.float32, device=self.device)
    self.eval_carry = torch.zeros(L, cw, dtype=torch.float32, device=self.device)   # evaluation acts between two fused steps: never the carry of a transition in flight
    new_box = (lambda: _MixedMailboxBlock(L, [w[0] for w in self.widths], [w[1] for w in self.widths])) if self.mixed else (lambda: _MailboxBlock(L, self.S, self.A))
    self._act_box, self._append_box, self._eval_box = new_box(), new_box(), new_box()
    self._seq = 0   # one sequence for the act and the append mailboxes: the device de-duplicates appends by commit word
    self._eval_seq = 0   # the evaluation mailboxes never post PENDING: a sequence of their own, so no number of evaluation launches between two appends can bring a learner's consumed word round again
    self._descs = {id(box): self._descriptors(box, carry) for box, carry in ((self._act_box, self.carry), (self._append_box, self.carry), (self._eval_box, self.eval_carry))}
    self._absorbing = np.array([bool(m.absorbing) for m in memories])
    self._all = list(range(L))
    self.reward_models = reward_models   # kept alive: the il_pwil_learner arrays below point into their atoms, weights and scratch
    self._reward_flag = REWARD_ON_DEVICE if reward_models is not None else 0
    if reward_models is not None:
      r0 = reward_models[0]
      for r in reward_models:
        assert (r.state_size, r.action_size) == (self.S, self.A) and _lib.on_device(r.expert_atoms), 'PopulationActingWorker(reward_models=...): the discriminators live on the GPU and have the rings\' dims'
        if (r.state_size, r.action_size, r.state_only, r.time_horizon) != (r0.state_size, r0.action_size, r0.state_only, r0.time_horizon):
          raise ValueError('PopulationActingWorker(reward_models=...): one state_size, action_size, state_only and time_horizon for all learners (they differ in their seed, i.e. in their atoms, alone)')
        r.require_device_coupling('PopulationActingWorker(reward_models=...)')   # NotImplementedError outside the one-launch coupling's sizes
      self._pwil_shape = max(reward_models, key=lambda r: r.expert_atoms.size(0))._desc   # the largest learner's descriptor: checked on the host, sizes the grid
      # one il_pwil_learner array per role; the act and the append mailboxes share the training carries. The evaluation mailboxes never post PENDING: no coupling
      self._pwil_descs = {id(box): self._pwil_descriptors(box) for box in (self._act_box, self._append_box)}

  def _descriptors(self, box: _MailboxBlock, carry: torch.Tensor) -> torch.Tensor:
    """The il_act_learner array of one role, uploaded once (every pointer is stable for the life of the worker)."""
    from .training import _device_array
    base, stride = box.tensor.data_ptr(), box.floats * 4
    return _device_array([_lib.ActLearner(a.flat.data_ptr(), base + l * stride, carry[l].data_ptr(), m.ring.data_ptr(), m._ring_state.data_ptr(), s & (2**64 - 1))
                          for l, (a, m, s) in enumerate(zip(self.actors, self.memories, self._seeds))], self.device)

  def _pwil_descriptors(self, box: _MailboxBlock) -> torch.Tensor:
    """The il_pwil_learner array of one role: every learner's own coupling descriptor with its mailbox of `box` and its training carry."""
    from .training import _device_array
    base, stride = box.tensor.data_ptr(), box.floats * 4
    return _device_array([_lib.PwilLearner(r._desc, base + l * stride, self.carry[l].data_ptr()) for l, r in enumerate(self.reward_models)], self.device)

  def _launch(self, box: _MailboxBlock, appends: bool = False):
    """`appends`: the launch may find pending transitions in `box` - with reward models their coupling launch goes first, on the same stream."""
    if appends and self.reward_models is not None:
      rc = _lib.lib().il_pwil_act_reward_population(_lib.ptr(self._pwil_descs[id(box)]), self.L, C.byref(self._pwil_shape), torch.cuda.current_stream().cuda_stream)
      if rc: _lib.check(rc)
    if self.mixed:
      rc = _lib.lib().il_act_step_population_mixed(_lib.ptr(self._descs[id(box)]), _lib.ptr(self._dims), C.cast(self._dims_host, C.c_void_p), self.L, self.H, torch.cuda.current_stream().cuda_stream)
    else:
      rc = _lib.lib().il_act_step_population(_lib.ptr(self._descs[id(box)]), self.L, self.S, self.A, self.H, torch.cuda.current_stream().cuda_stream)
    if rc: _lib.check(rc)

  def _next_seq(self) -> int:
    self._seq = self._seq % (_SEQ_MOD - 1) + 1
    return self._seq

  def _next_eval_seq(self) -> int:
    self._eval_seq = self._eval_seq % (_SEQ_MOD - 1) + 1
    return self._eval_seq

  def _post_act(self, box: _MailboxBlock, obs, flags: np.ndarray):
    """Observation and Philox offset of every learner that acts (flags without NO_ACTION); counts the act in its actor, as SoftActor._act does."""
    rows = [l for l in self._all if not flags[l] & NO_ACTION]
    if rows:
      if self.mixed:
        for l in rows: box.host[l, box.o_obs[l]:box.o_obs[l] + self.S[l]] = _row(obs[l])[:self.S[l]]
      else:
        box.host[rows, box.o_obs:box.o_obs + self.S] = _rows(obs, rows, self.S)
      calls = []
      for l in rows:
        a = self.actors[l]
        a._act_calls += 1   # the Philox offset is shared with SoftActor._act, so the two entry points never reuse noise
        calls.append(a._act_calls & 0xFFFFFFFF)
      box.bits[rows, _NOISE_OFFSET] = calls

  def _post_transition(self, box: _MailboxBlock, rows, step, next_obs, reward, terminal, timeout):
    if rows:
      box.host[rows, 2:6] = np.array([(float(reward[l]), float(bool(terminal[l])), float(bool(timeout[l])), float(step[l] if np.ndim(step) else step)) for l in rows], dtype=np.float32)
      if self.mixed:
        for l in rows: box.host[l, box.o_next:box.o_next + self.S[l]] = _row(next_obs[l])[:self.S[l]]
      else:
        box.host[rows, box.o_next:box.o_next + self.S] = _rows(next_obs, rows, self.S)

  def _mirror_appends(self, rows, terminal, timeout, wrap):
    for l in rows:
      m = self.memories[l]
      m._advance(bool(terminal[l]), bool(timeout[l]))
      if wrap[l]: m._advance(False, False)

  def _collect(self, box: _MailboxBlock) -> torch.Tensor:
    box.wait('il_act_step_population')
    if self.mixed:   # [L, widest A]: row l holds learner l's A_l components, zeros behind them
      out = np.zeros((self.L, self.A), dtype=np.float32)
      for l, (_, A) in enumerate(self.widths): out[l, :A] = box.host[l, box.o_act[l]:box.o_act[l] + A]
      return torch.from_numpy(out)
    return torch.from_numpy(box.host[:, box.o_act:box.o_act + self.A].copy())

  def _transition_flags(self, next_obs, terminal, timeout):
    rows = [l for l in self._all if next_obs[l] is not None]
    wrap = np.zeros(self.L, dtype=bool)
    for l in rows:
      wrap[l] = self._absorbing[l] and bool(terminal[l]) and not bool(timeout[l])
    flags = np.zeros(self.L, dtype=np.int64)
    flags[rows] = PENDING | self._reward_flag
    flags[wrap] |= WRAP_ABSORBING
    return rows, wrap, flags

  # --- exact schedule
  def act(self, obs, greedy: bool = False, _box=None) -> torch.Tensor:
    """`actor_l(obs[l]).sample()` (or the greedy action) for every learner as one [L, A] CPU tensor, remembering (obs, action) on the device for `append`. `obs[l] is None`:
    learner l idles (its row of the result is whatever its mailbox last held)."""
    box = _box or self._act_box
    flags = np.array([NO_ACTION if o is None else (GREEDY if greedy else 0) for o in obs], dtype=np.int64)
    assert len(flags) == self.L
    self._post_act(box, obs, flags)
    box.commit(self._next_eval_seq() if box is self._eval_box else self._next_seq(), flags)
    self._launch(box)
    return self._collect(box)

  def append(self, step, next_obs, reward, terminal, timeout):
    """`memory_l.append(...)` of the (state, action) of learner l's last `act`, plus its absorbing wrap at a true termination. Asynchronous: nothing is waited for.
    `step`: one int for all learners or a list; `next_obs[l] is None`: learner l idles. With reward models the ring's reward is the device's (`reward` is the caller's,
    e.g. for its train_return), here and in `step`."""
    box = self._append_box
    if box.words is not None: box.wait('il_act_step_population(append)')   # normally already echoed: the act in between ran after it on the same stream
    rows, wrap, flags = self._transition_flags(next_obs, terminal, timeout)
    flags |= NO_ACTION
    self._post_transition(box, rows, step, next_obs, reward, terminal, timeout)
    box.commit(self._next_seq(), flags)
    self._launch(box, appends=True)
    self._append_launched = True
    self._mirror_appends(rows, terminal, timeout, wrap)

  def __del__(self):
    _drain(getattr(self, '_append_box', None), getattr(self, '_append_launched', False), 'il_act_step_population(append)')

  # --- fused schedule
  def step(self, step, next_obs, reward, terminal, timeout, obs=None, greedy: bool = False) -> torch.Tensor:
    """append(transition of learner l's last action) + act(obs[l]) for every learner in ONE launch. `obs[l]` defaults to `next_obs[l]`; pass the reset observation where
    the episode ended. `next_obs[l] is None`: learner l idles (no append, no action)."""
    box = self._act_box
    rows, wrap, flags = self._transition_flags(next_obs, terminal, timeout)
    idle = [l for l in self._all if next_obs[l] is None]
    flags[idle] = NO_ACTION
    if greedy: flags[rows] |= GREEDY
    self._post_transition(box, rows, step, next_obs, reward, terminal, timeout)
    self._post_act(box, [None if next_obs[l] is None else (next_obs[l] if obs is None or obs[l] is None else obs[l]) for l in self._all], flags)
    box.commit(self._next_seq(), flags)
    self._launch(box, appends=True)
    self._mirror_appends(rows, terminal, timeout, wrap)
    return self._collect(box)

  # --- evaluation: the same kernel through a second descriptor set (own mailboxes, scratch carries, never PENDING)
  def act_eval(self, obs) -> torch.Tensor:
    """Greedy actions for the learners with an observation ([L, A]; the others idle), leaving the training carries and mailboxes alone."""
    return self.act(obs, greedy=True, _box=self._eval_box)
