"""Greedy-policy evaluation: same call and return shape as the reference's evaluate_agent (evaluation.py:11-35).

The policy mean comes from `il_actor_act` (one launch per environment step, SoftActor.get_greedy_action); the environment and the
episode bookkeeping stay on the host, as in the reference. Episodes are recorded into preallocated host buffers (the horizon is
known from env.max_episode_steps) instead of python lists of 1-row tensors.

`evaluate_population` evaluates the L learners of a `PopulationActingWorker` in lockstep: one `il_act_step_population` launch per evaluation step for all of them.

`evaluate_agent_lockstep` / `evaluate_population_lockstep` (`+evaluation.schedule=lockstep`) step ALL episodes of an evaluation in lockstep, one seeded environment per
episode: one `il_act_eval_rows` launch per lockstep step for every row of every learner (`LockstepEvaluator`; general actor shapes: `il_act_eval_rows_general`,
`GeneralLockstepEvaluator`). Their returns are those of E seeded copies of the evaluation
environment, not of one environment stepped E times; `evaluate_agent` and `evaluate_population` are what they were.
"""
import torch


class _EpisodeLog:
  """Host-side record of one evaluation episode."""

  def __init__(self, horizon: int, keep_steps: bool):
    self.keep_steps, self.length, self.total = keep_steps, 0, 0.0
    self.reward = torch.zeros(horizon, dtype=torch.float32)
    self.state = self.action = None

  def push(self, state, action, reward: float):
    t = self.length
    if t >= self.reward.numel():  # environments without a declared horizon: grow geometrically
      self.reward = torch.cat([self.reward, torch.zeros_like(self.reward)])
      if self.state is not None:
        self.state, self.action = torch.cat([self.state, torch.zeros_like(self.state)]), torch.cat([self.action, torch.zeros_like(self.action)])
    if self.keep_steps:
      if self.state is None:
        self.state = torch.zeros(self.reward.numel(), state.shape[-1]); self.action = torch.zeros(self.reward.numel(), action.shape[-1])
      self.state[t], self.action[t] = state.reshape(-1).cpu(), action.reshape(-1).cpu()
    self.reward[t] = reward
    self.total += float(reward)
    self.length = t + 1

  def as_trajectory(self):
    n = self.length
    done = torch.zeros(n); done[n - 1] = 1.0
    return dict(states=self.state[:n].clone(), actions=self.action[:n].clone(), rewards=self.reward[:n].clone(), terminals=done)


def evaluate_agent(actor, env, num_episodes: int, return_trajectories: bool = False, render: bool = False):
  horizon = int(getattr(env, 'max_episode_steps', 0) or 1024)
  logs = []
  with torch.inference_mode():
    for _ in range(num_episodes):
      log, obs, finished = _EpisodeLog(horizon, return_trajectories), env.reset(), False
      while not finished:
        act = actor.get_greedy_action(obs)
        nxt, r, finished = env.step(act)
        log.push(obs, act, r)
        obs = nxt
      logs.append(log)
  returns = [log.total for log in logs]
  if return_trajectories:
    return returns, [log.as_trajectory() for log in logs]
  return returns


def _lockstep_logs(evaluator, envs_per_learner, num_episodes: int, keep_steps: bool):
  """All `num_episodes` evaluation episodes of every learner in lockstep: episode k of learner l runs on envs_per_learner[l][k], and every lockstep step is ONE
  `LockstepEvaluator.act` (one launch) for the rows of all episodes still running. An episode that has finished leaves its learner's row set - the rows are compacted here,
  on the host, in episode order. Returns the episode logs per learner, in episode order."""
  L = evaluator.L
  assert len(envs_per_learner) == L, f'one list of environments per learner ({L}), got {len(envs_per_learner)}'
  E = int(num_episodes)
  if E <= 0: return [[] for _ in range(L)]
  for l, envs in enumerate(envs_per_learner):
    assert len(envs) >= E, f'lockstep evaluation of {E} episodes needs {E} environments per learner (learner {l} has {len(envs)})'
  assert E <= evaluator.max_rows, f'lockstep evaluation of {E} episodes needs an evaluator of max_rows >= {E} (it has {evaluator.max_rows})'
  with torch.inference_mode():
    logs = [[_EpisodeLog(int(getattr(envs[k], 'max_episode_steps', 0) or 1024), keep_steps) for k in range(E)] for envs in envs_per_learner]
    obs = [[envs[k].reset() for k in range(E)] for envs in envs_per_learner]
    live = [list(range(E)) for _ in range(L)]
    while any(live):
      acts = evaluator.act([[obs[l][k] for k in live[l]] for l in range(L)])
      for l in range(L):
        still = []
        for i, k in enumerate(live[l]):
          act = acts[l][i:i + 1]
          nxt, r, finished = envs_per_learner[l][k].step(act)
          logs[l][k].push(obs[l][k], act, r)
          obs[l][k] = nxt
          if not finished: still.append(k)
        live[l] = still
  return logs


def evaluate_agent_lockstep(actor, envs, num_episodes: int, return_trajectories: bool = False, evaluator=None):
  """`evaluate_agent`'s call and return shape with the episodes in lockstep: episode k runs on envs[k], and one lockstep step of all of them is ONE `il_act_eval_rows` launch
  (`il.LockstepEvaluator`; pass one to reuse its mailbox across evaluations, it must serve `actor` alone) instead of one `get_greedy_action` turn-around per episode and
  step. Per row the action is `get_greedy_action`'s, bit for bit, so episode k's return is what `evaluate_agent(actor, envs[k], 1)` gives - the returns are those of
  `num_episodes` seeded environments, NOT those of one environment stepped `num_episodes` times. `actor._act_calls` advances by the steps taken."""
  if evaluator is None:   # a general actor shape: il_act_eval_rows_general (per row il_actor_act_general's greedy action, which is what its get_greedy_action runs)
    from .acting import GeneralLockstepEvaluator, LockstepEvaluator
    evaluator = (GeneralLockstepEvaluator if getattr(actor, 'general', False) else LockstepEvaluator)([actor], max(int(num_episodes), 1))
  assert evaluator.L == 1 and evaluator.actors[0] is actor, 'evaluate_agent_lockstep: the evaluator serves this actor alone (several learners: evaluate_population_lockstep)'
  logs = _lockstep_logs(evaluator, [envs], num_episodes, return_trajectories)[0]
  returns = [log.total for log in logs]
  if return_trajectories:
    return returns, [log.as_trajectory() for log in logs]
  return returns


def evaluate_population_lockstep(evaluator, envs_per_learner, num_episodes: int):
  """`[evaluate_agent_lockstep(actor_l, envs_per_learner[l], num_episodes) for l]` with ONE launch per lockstep step for the rows of all L learners (the learner is a grid
  axis of `il_act_eval_rows`). A learner whose episodes have all finished idles until the last one has."""
  return [[log.total for log in logs] for logs in _lockstep_logs(evaluator, envs_per_learner, num_episodes, False)]


def evaluate_population(worker, eval_envs, num_episodes: int):
  """`[evaluate_agent(actor_l, eval_envs[l], num_episodes) for l]` with ONE launch per lockstep evaluation step (`PopulationActingWorker.act_eval`: greedy, own mailboxes
  and scratch carries, so a transition in flight between two fused steps keeps its carry). A learner that has finished its episodes idles until the last one has; each
  actor's `_act_calls` advances by the number of steps of its own episodes, as `get_greedy_action` would have advanced it."""
  L = worker.L
  assert len(eval_envs) == L
  returns = [[] for _ in range(L)]
  if num_episodes <= 0: return returns
  widths = worker.widths if getattr(worker, 'mixed', False) else None   # learners of different widths: row l of the [L, widest A] actions holds learner l's own A_l components
  with torch.inference_mode():
    obs, totals = [env.reset() for env in eval_envs], [0.0] * L
    while any(o is not None for o in obs):
      acts = worker.act_eval(obs)
      for l in range(L):
        if obs[l] is None: continue
        nxt, r, finished = eval_envs[l].step(acts[l:l + 1, :widths[l][1]] if widths else acts[l:l + 1])
        totals[l] += float(r)
        if finished:
          returns[l].append(totals[l]); totals[l] = 0.0
          nxt = eval_envs[l].reset() if len(returns[l]) < num_episodes else None
        obs[l] = nxt
  return returns
