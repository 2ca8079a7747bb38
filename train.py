#!/usr/bin/env python3
"""Entry point with the reference's command line:  python train.py algorithm=<ALG> env=<ENV> [key.sub=value ...]

Drives the loop of reference train.py:26-243 (act -> store -> [update block] -> evaluate -> save) on the MI355X path:
the update block (train.py:171-203) is `UpdatePlan` (one captured hipGraph replay per step, every algorithm) or the per-function HIP entry
points (GAIL variants with per-update host inputs, batch sizes that are not a multiple of 16 - where the default networks run csrc/general.hip).  Hydra is replaced by `imitation_learning_amd.config.compose`
(same keys, same precedence).  Supported on the HIP path: SAC, GAIL (BCE loss), GMMIL, PWIL, AdRIL (and SQIL via update_freq=0), RED, DRIL, BC - every algorithm= of the reference.
Acting goes through `il.ActingWorker` for every algorithm (`+acting.schedule=exact|fused|overlap`, default exact; `per_function` keeps the reference's call sequence). PWIL's
reward is computed on the device in front of each append and its expert relabel (mix_expert_data != none) is one library call; `+pretraining.schedule=per_function` keeps
the row-by-row loop.

Sweeps:  python train.py -m seed=1,2,3 algorithm=GAIL env=halfcheetah  (Hydra's multirun: comma lists, Cartesian product, outputs/<algorithm>_<env>_sweeper/<time>/<job>/).
Jobs that differ only in their seed train as ONE population in lockstep (`train_sweep`: `il.BatchedPopulationPlan` for the update, `il.PopulationActingWorker` or one
`il.ActingWorker` per learner for acting: `+sweep.schedule=population|per_learner`, the same bits either way; GMMIL and DRIL sweeps only when that key is given, PWIL sweeps only under `+sweep.pwil_population=true`:
one `il_pwil_act_reward_population` coupling launch per lockstep step in front of the population acting launch, AdRIL / SQIL sweeps only under `+sweep.adril_population=true`:
one `il_batch_mix_relabel_population` launch per update between the gathers and the SAC launches, GAIL sweeps whose loss is Mixup (the `GAIL_5_trajectories` and
`GAIL_10_trajectories` overlays) only under `+sweep.gail_mixup_population=true`: `il_gail_mixup_step_population`, at any `mixup_alpha`, every learner's coefficients under
its own Philox key and update counter); every other sweep runs its jobs one after another, and says so.

Evaluation: `+evaluation.schedule=sequential` (default: evaluate_agent / evaluate_population, unchanged) or `lockstep` - `evaluation.episodes` seeded copies of the evaluation
environment per learner (copy k seeded seed + 7919 k, copy 0 the sequential schedule's), all episodes stepped together with ONE il_act_eval_rows launch per lockstep step
(il.LockstepEvaluator; a general actor shape inside the one-launch tile engine: il_act_eval_rows_general, il.GeneralLockstepEvaluator). Lockstep returns are those of the E
copies, not of one environment stepped E times; where neither launch serves the run a `[train] evaluation:` line says why.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imitation_learning_amd as il  # noqa: E402
from imitation_learning_amd import _lib  # noqa: E402
from imitation_learning_amd import config as il_config  # noqa: E402
from imitation_learning_amd.config import EVALUATION_SCHEDULES, eval_env_seed, evaluation_schedule  # noqa: E402,F401
from imitation_learning_amd.environments import env_dims, make_env  # noqa: E402
from imitation_learning_amd.evaluation import evaluate_agent, evaluate_agent_lockstep, evaluate_population, evaluate_population_lockstep  # noqa: E402
from imitation_learning_amd.models import default_device  # noqa: E402
from imitation_learning_amd.utils import cycle, lineplot  # noqa: E402


def expert_batches(cfg, expert_memory, state_size, action_size, count):
  """`count` shuffled, drop-last minibatches of the expert memory, reshuffled every epoch (the cycle(DataLoader(...)) of train.py:94,116)."""
  B, n = cfg.training.batch_size, expert_memory.size
  assert n >= B, f'pretraining needs at least one full batch of expert data ({n} < {B})'
  shuffle = torch.Generator().manual_seed(cfg.seed)
  while count > 0:
    order = torch.randperm(n, generator=shuffle).to(torch.int32)
    for lo in range(0, min(n - B + 1, count * B), B):
      yield il.memory.batch_views(expert_memory.gather(order[lo:lo + B]), state_size, action_size, cfg.imitation.absorbing)
      count -= 1


def pretraining_schedule(cfg) -> str:
  """'plan' (default): the expert-data loops run as a device-resident epoch (il.PretrainPlan: one library call per few thousand iterations). `+pretraining.schedule=per_function`
  keeps the loop over `expert_batches` below - one gather and one per-function update per iteration - as the reference and for A/B runs; both leave the same bits."""
  schedule = (cfg.get('pretraining', {}) or {}).get('schedule', 'plan')
  assert schedule in ('plan', 'per_function')
  return schedule


def pretrain_bc(cfg, actor, expert_memory, state_size, action_size):
  """cfg.bc_pretraining.iterations steps of behavioural cloning (train.py:93-100)."""
  optimiser = il.AdamW(actor, lr=cfg.bc_pretraining.learning_rate, weight_decay=cfg.bc_pretraining.weight_decay)
  if pretraining_schedule(cfg) == 'plan':
    il.PretrainPlan('BC', actor, optimiser, expert_memory, cfg.training.batch_size, torch.Generator().manual_seed(cfg.seed)).run(cfg.bc_pretraining.iterations)
    return
  for batch in expert_batches(cfg, expert_memory, state_size, action_size, cfg.bc_pretraining.iterations):
    il.behavioural_cloning_update(actor, batch, optimiser)


class _Learner:
  """Everything one learner owns: train() has one, a seed sweep one per job."""


def new_metrics() -> dict:
  return dict(train_steps=[], train_returns=[], test_steps=[], test_returns=[], test_returns_normalized=[], update_steps=[], predicted_rewards=[], alphas=[], entropies=[], Q_values=[])


def build_agent(ln, cfg, state_size, action_size, dev):
  """Actor, critic, target, the three optimisers and the replay memory of one learner, as attributes of `ln` - in the order that consumes the process seed, which the
  caller has set in front."""
  ln.actor, ln.critic, ln.log_alpha = il.SoftActor(state_size, action_size, cfg.reinforcement.actor), il.TwinCritic(state_size, action_size, cfg.reinforcement.critic), torch.zeros(1, device=dev)
  ln.target_critic, ln.entropy_target = il.create_target_network(ln.critic), cfg.reinforcement.target_temperature * action_size
  ln.actor_optimiser = il.AdamW(ln.actor, lr=cfg.training.learning_rate, weight_decay=cfg.training.weight_decay)
  ln.critic_optimiser = il.AdamW(ln.critic, lr=cfg.training.learning_rate, weight_decay=cfg.training.weight_decay)
  ln.temperature_optimiser = il.Adam(ln.log_alpha, lr=cfg.training.learning_rate)
  ln.memory = il.ReplayMemory(cfg.memory.size, state_size, action_size, cfg.imitation.absorbing)


def build_reward_model(cfg, state_size, action_size, expert_memory, max_episode_steps):
  """(discriminator, its optimiser) of cfg.algorithm, built behind the agent; (None, None) for SAC and BC."""
  with_optimiser = lambda d: (d, il.AdamW(d, lr=cfg.imitation.learning_rate, weight_decay=cfg.imitation.weight_decay))
  if cfg.algorithm == 'AdRIL':   # no parameters: its state is the balanced alternation (update_freq=0: SQIL)
    return il.RewardRelabeller(cfg.imitation.update_freq, cfg.imitation.balanced), None
  if cfg.algorithm == 'GAIL':
    return with_optimiser(il.GAILDiscriminator(state_size, action_size, cfg.imitation, cfg.reinforcement.discount))
  if cfg.algorithm == 'GMMIL':   # no parameters and no optimiser: its state is the two bandwidths the learner's first batch fixes
    return il.GMMILDiscriminator(state_size, action_size, cfg.imitation), None
  if cfg.algorithm == 'PWIL':   # the learner's own atoms: its expert data was subsampled under its seed
    return il.PWILDiscriminator(state_size, action_size, cfg.imitation, expert_memory, max_episode_steps), None
  if cfg.algorithm == 'DRIL':   # dropout policy ensemble (train.py:73 builds it as SoftActor(...))
    return with_optimiser(il.DropoutSoftActor(state_size, action_size, cfg.imitation.discriminator))
  if cfg.algorithm == 'RED':
    return with_optimiser(il.REDDiscriminator(state_size, action_size, cfg.imitation))
  return None, None


def pretrain_reward_model(cfg, discriminator, discriminator_optimiser, expert_memory, state_size, action_size):
  """train.py:114-134 for DRIL and RED: pretrain the "discriminator" on expert data, then fix its reward threshold / bandwidth. Runs while the learner's seed is the
  process seed (the DRIL ensemble's descriptors read their Philox key from it)."""
  B = cfg.training.batch_size
  if pretraining_schedule(cfg) == 'plan' and cfg.imitation.pretraining.iterations > 0:
    il.PretrainPlan(cfg.algorithm, discriminator, discriminator_optimiser, expert_memory, B, torch.Generator().manual_seed(cfg.seed)).run(cfg.imitation.pretraining.iterations)
  else:
    for batch in expert_batches(cfg, expert_memory, state_size, action_size, cfg.imitation.pretraining.iterations):
      if cfg.algorithm == 'DRIL': il.behavioural_cloning_update(discriminator, batch, discriminator_optimiser)
      else: il.target_estimation_update(discriminator, batch, discriminator_optimiser)
  if cfg.algorithm == 'DRIL': discriminator.set_uncertainty_threshold(expert_memory['states'][:expert_memory.size], expert_memory['actions'][:expert_memory.size], cfg.imitation.quantile_cutoff)
  else: discriminator.set_sigma(expert_memory['states'][:B], expert_memory['actions'][:B])


def relabel_row_by_row(discriminator, expert_memory):
  """PWIL's expert relabel (train.py:135-141) as the reference's loop, a host round trip per row: `+pretraining.schedule=per_function` (A/B runs) and atom sets outside
  the one-launch coupling; the same bits as PWILDiscriminator.relabel_memory."""
  for i in range(expert_memory.size):
    tr = expert_memory[i]
    expert_memory.rewards[i] = discriminator.compute_reward(tr['states'].unsqueeze(0), tr['actions'].unsqueeze(0))
    if tr['terminals'] or tr['timeouts']: discriminator.reset()


def record_evaluation(cfg, metrics, prefix, step, episode_returns, normalised):
  """One evaluation into the metrics, and the plots of train.py:216-228."""
  for key, value in (('test_steps', step), ('test_returns', episode_returns), ('test_returns_normalized', list(normalised))): metrics[key].append(value)
  lineplot(metrics['test_steps'], metrics['test_returns'], filename=f'{prefix}test_returns', title=f'{cfg.algorithm}: {cfg.env} Test Returns')
  if len(metrics['train_returns']) > 0:
    lineplot(metrics['train_steps'], metrics['train_returns'], filename=f'{prefix}train_returns', title=f'Training {cfg.algorithm}: {cfg.env} Train Returns')
  if cfg.logging.interval > 0 and len(metrics['update_steps']) > 0:   # train.py:224-228
    if cfg.algorithm != 'SAC': lineplot(metrics['update_steps'], metrics['predicted_rewards'], filename=f'{prefix}predicted_rewards', yaxis='Predicted Reward', title=f'{cfg.algorithm}: {cfg.env} Predicted Rewards')
    lineplot(metrics['update_steps'], metrics['alphas'], filename=f'{prefix}sac_alpha', yaxis='Alpha', title=f'{cfg.algorithm}: {cfg.env} Alpha')
    lineplot(metrics['update_steps'], metrics['entropies'], filename=f'{prefix}sac_entropy', yaxis='Entropy', title=f'{cfg.algorithm}: {cfg.env} Entropy')
    lineplot(metrics['update_steps'], metrics['Q_values'], filename=f'{prefix}Q_values', yaxis='Q-value', title=f'{cfg.algorithm}: {cfg.env} Q-values')


def lockstep_eval_envs(cfg, seed: int, eval_env, env_kw) -> list:
  """The `evaluation.episodes` evaluation environments of one learner under +evaluation.schedule=lockstep: `eval_env` (already seeded with `seed`) is copy 0, the others
  are built here and seeded by eval_env_seed. They persist across the evaluations of a run, like eval_env."""
  envs = [eval_env]
  for k in range(1, max(int(cfg.evaluation.episodes), 1)):
    env = make_env(cfg.env, cfg.imitation.absorbing, **env_kw)
    env.seed(eval_env_seed(seed, k))
    envs.append(env)
  return envs


def lockstep_evaluator(cfg, actors, each: bool = False):
  """An evaluator for `actors` (`each`: a list of them, one per actor - the per_learner sweep schedule) when +evaluation.schedule=lockstep asks for one: an
  il.LockstepEvaluator when il_act_eval_rows serves them all (the fused actor shape); when it refuses, an il.GeneralLockstepEvaluator, built the same way, when
  il_act_eval_rows_general does (general shapes inside the one-launch tile engine: hidden a multiple of 16 up to 512, state <= 512, action <= 8, one shape for all).
  Otherwise None - under `lockstep` with ONE `[train] evaluation:` line for the run that gives both reasons (a shape only the layer-at-a-time kernels run,
  IL_GENERAL_TILES=0, fused and general actors mixed, more than 1,024 episodes): the run then evaluates sequentially, every learner of it."""
  if evaluation_schedule(cfg) != 'lockstep': return None
  rows = max(int(cfg.evaluation.episodes), 1)
  build = lambda cls: [cls([a], rows) for a in actors] if each else cls(actors, rows)
  try:
    return build(il.LockstepEvaluator)
  except NotImplementedError as fused:
    try:
      return build(il.GeneralLockstepEvaluator)
    except NotImplementedError as general:
      print(f'[train] evaluation: +evaluation.schedule=lockstep cannot be served: {fused}; {general}; evaluating under the sequential schedule', file=sys.stderr)
      return None


def save_run(cfg, prefix, metrics, actor, critic, log_alpha, discriminator, eval_env, lockstep=None):
  """What a finished run leaves behind (train.py:231-240). `lockstep`: (evaluator, environments) - the trajectories then come from evaluate_agent_lockstep (which, like
  evaluate_agent here, renders nothing: `cfg.render` has no effect on either path)."""
  if cfg.save_trajectories and lockstep is not None:
    _, trajectories = evaluate_agent_lockstep(actor, lockstep[1], cfg.evaluation.episodes, return_trajectories=True, evaluator=lockstep[0])
    torch.save(trajectories, f'{prefix}trajectories.pth')
  elif cfg.save_trajectories:   # train.py:231-234
    _, trajectories = evaluate_agent(actor, eval_env, cfg.evaluation.episodes, return_trajectories=True, render=cfg.render)
    torch.save(trajectories, f'{prefix}trajectories.pth')
  torch.save(dict(actor=actor.state_dict(), critic=critic.state_dict(), log_alpha=log_alpha), f'{prefix}agent.pth')
  if cfg.algorithm in ('DRIL', 'GAIL', 'RED'): torch.save(discriminator.state_dict(), f'{prefix}discriminator.pth')   # train.py:238
  torch.save(metrics, f'{prefix}metrics.pth')


def check_timeouts_seen(plan, step, last_good):
  """Every update step, no synchronisation: the pinned host words a device-side wait stores into when it gives up (UpdatePlan.watch_timeouts). Raises within the pipeline
  depth of the expiry (one or two updates), naming the last step at which the words still read zero - checkpoints are only ever written after a clean check."""
  handoff, exchange = plan.timeouts_seen()
  if handoff or exchange:
    what = (f'{exchange} wait(s) of the peer-window gradient exchange (a rank did not deliver its gradients within the bound: IL_PEER_EXCHANGE=0 selects RCCL all-reduces)' if exchange else
            f'{handoff} device-side hand-off wait(s) (the discriminator and SAC branches did not run concurrently: IL_DEVICE_SYNC=0 selects stream dependencies)')
    raise RuntimeError(f'step {step}: {what} expired; updates since step {last_good} (the last one checked clean) may have trained on stale rewards / gradients. Nothing was saved after that step.')


def check_handoff(plan, step, runner=None):
  """The two branches of a captured GAIL update hand over through device counters with BOUNDED waits (include/il_hip.h il_sync): a wait that expires lets the
  update proceed on stale rewards / discriminator weights and bumps a counter. That can only happen if something stops the two streams from running
  concurrently after `capture()` validated them (a profiler attached mid-run, a CU mask, a co-tenant process). Training on such updates silently is worse
  than stopping: raise, naming the switch that trades the hand-off for plain stream dependencies."""
  n = runner.exchange_timeouts() if hasattr(runner, 'exchange_timeouts') else 0
  if n:
    raise RuntimeError(f'step {step}: {n} device-side waits of the peer-window gradient exchange expired since set-up - a rank did not deliver its gradients within the bound, '
                       'so some update averaged stale slabs and the replicas may have diverged. Re-run with IL_PEER_EXCHANGE=0 (RCCL all-reduces).')
  if plan is None or not getattr(plan, 'device_sync', False): return
  n = plan.sync_timeouts()
  if n:
    raise RuntimeError(f'step {step}: {n} device-side hand-off waits expired since the last check - the discriminator and SAC branches of the update did not run concurrently, '
                       'so updates in this interval used stale rewards. Re-run with IL_DEVICE_SYNC=0 (stream dependencies instead of device counters).')


def train(cfg, file_prefix: str = '') -> float:
  il_config.validate(cfg)
  evaluation_schedule(cfg)   # an unknown +evaluation.schedule stops the run here, on every rank
  # ---- data parallelism (BASELINE.json configs[4]): one process per GPU, own environment + replay shard, replicated networks, three gradient
  # all-reduces per update. Launched by torch.distributed.run; rank r seeds everything with seed + r (its data must differ), parameters come from rank 0.
  world = int(cfg.distributed.world_size)
  rank = 0
  if world > 1:
    from imitation_learning_amd import parallel
    assert torch.cuda.is_available(), 'train.py needs a GPU: the update path has no CPU fallback'
    rank, _, dev = parallel.init_from_env(world, cfg.distributed.backend)
    dog = parallel.Watchdog(float(cfg.distributed.timeout_s), what=f'train.py (rank {rank} of {world})', armed=False)   # a rank that dies inside a collective must not hang the others; armed at the first captured update (the set-up phases before it have no bound of their own)
  else:
    dev, dog = default_device(), None
  assert _lib.on_device(torch.empty(0, device=dev)), 'train.py needs a GPU: the update path has no CPU fallback'
  lead = rank == 0                # evaluation, plots and checkpoints are rank 0's job
  seed = cfg.seed + rank
  il.seed(seed)                   # replay index stream (np.random.seed in the reference, train.py:51)
  np.random.seed(seed)
  torch.manual_seed(seed)

  env_kw = dict(cfg.get('synthetic_env', {}) or {})
  env, eval_env = make_env(cfg.env, cfg.imitation.absorbing, load_data=True, **env_kw), make_env(cfg.env, cfg.imitation.absorbing, **env_kw)
  env.seed(seed); eval_env.seed(seed)
  score_lo, score_hi = env.env.ref_min_score, env.env.ref_max_score
  normalise = lambda returns: (np.asarray(returns) - score_lo) / (score_hi - score_lo)  # D4RL normalised score
  expert_memory = env.get_dataset(trajectories=cfg.imitation.trajectories, subsample=cfg.imitation.subsample, device=dev)
  state_size, action_size = env.observation_space.shape[0], env.action_space.shape[0]

  ln = _Learner()
  build_agent(ln, cfg, state_size, action_size, dev)
  actor, critic, log_alpha, target_critic, entropy_target, memory = ln.actor, ln.critic, ln.log_alpha, ln.target_critic, ln.entropy_target, ln.memory
  actor_optimiser, critic_optimiser, temperature_optimiser = ln.actor_optimiser, ln.critic_optimiser, ln.temperature_optimiser
  discriminator, discriminator_optimiser = build_reward_model(cfg, state_size, action_size, expert_memory, env.max_episode_steps)

  if world > 1:   # replicas start from rank 0's initialisation (the per-rank torch seeds differ)
    parallel.broadcast_parameters(parallel.replica_tensors(actor, critic, target_critic, log_alpha, discriminator))
  # +evaluation.schedule=lockstep: one seeded copy of the evaluation environment per evaluation episode and one launch per lockstep step (rank 0 evaluates)
  evaluator = lockstep_evaluator(cfg, [actor]) if lead else None
  lockstep = (evaluator, lockstep_eval_envs(cfg, seed, eval_env, env_kw)) if evaluator is not None else None
  evaluate = (lambda: evaluate_agent_lockstep(actor, lockstep[1], cfg.evaluation.episodes, evaluator=evaluator)) if lockstep is not None else \
             (lambda: evaluate_agent(actor, eval_env, cfg.evaluation.episodes))
  metrics = new_metrics()
  score = []
  if cfg.check_time_usage: start_time = time.time()
  B = cfg.training.batch_size

  # ---- behavioural cloning pretraining (train.py:93-112)
  if cfg.bc_pretraining.iterations > 0:
    pretrain_bc(cfg, actor, expert_memory, state_size, action_size)
    if cfg.algorithm == 'BC':
      if cfg.check_time_usage: metrics['pre_training_time'] = time.time() - start_time
      episode_returns = evaluate()
      normalised = normalise(episode_returns)
      metrics.update(test_steps=[0], test_returns=[episode_returns], test_returns_normalized=[list(normalised)])
      if world > 1:   # algorithm=BC has no update block to parallelise: every rank clones on its own, rank 0 reports
        torch.distributed.barrier(); torch.distributed.destroy_process_group(); dog.stop()
      if not lead: return float(np.mean(normalised))
      torch.save(dict(actor=actor.state_dict()), f'{file_prefix}agent.pth')
      torch.save(metrics, f'{file_prefix}metrics.pth')
      return float(np.mean(normalised))

  if cfg.algorithm in ('DRIL', 'RED'):  # train.py:114-134: pretrain the "discriminator" on expert data, then fix its reward threshold / bandwidth
    pretrain_reward_model(cfg, discriminator, discriminator_optimiser, expert_memory, state_size, action_size)
    if cfg.check_time_usage: metrics['pre_training_time'], start_time = time.time() - start_time, time.time()
    if cfg.imitation.mix_expert_data == 'prefill_memory': memory.transfer_transitions(expert_memory)

  if world > 1 and (cfg.bc_pretraining.iterations > 0 or cfg.algorithm in ('DRIL', 'RED')):   # every rank pretrained on its own shuffles: keep rank 0's result
    parallel.broadcast_parameters(parallel.replica_tensors(actor, critic, target_critic, log_alpha, discriminator))
    if cfg.algorithm == 'DRIL': discriminator.q, = parallel.broadcast_scalars([discriminator.q])
    if cfg.algorithm == 'RED': discriminator.sigma_1, = parallel.broadcast_scalars([discriminator.sigma_1])

  if cfg.algorithm == 'PWIL' and cfg.imitation.mix_expert_data != 'none':  # train.py:135-141
    relabelled = False
    if pretraining_schedule(cfg) == 'plan':   # one library call: a coupling launch per row, the weights set back on the device after every trajectory's last row
      try:
        discriminator.relabel_memory(expert_memory)
        relabelled = True
      except NotImplementedError as e:   # an atom set outside the one-launch coupling's sizes: the loop below
        print(f'[train] {e}; relabelling the expert memory row by row', file=sys.stderr)
    if not relabelled: relabel_row_by_row(discriminator, expert_memory)
  if cfg.algorithm in ('PWIL', 'GMMIL') and cfg.imitation.mix_expert_data == 'prefill_memory':
    memory.transfer_transitions(expert_memory)

  # ---- the update block as ONE captured graph per step (UpdatePlan) whenever its inputs are device-resident; otherwise the per-function entry points
  plan = None
  mixed = cfg.imitation.mix_expert_data == 'mixed_batch'
  fusable = B % 16 == 0
  if cfg.algorithm == 'GAIL' and (mixed or cfg.imitation.bc_aux_loss):
    fusable = False   # a mix between the discriminator step and the relabel / an auxiliary actor step on the expert batch: per-function path. (Every discriminator variant -
    # loss functions, finite PUGAIL margin, subtract_log_policy, reward shaping, depth 2 / tanh, Mixup with any alpha - is captured by UpdatePlan.)
  if fusable:
    plan = il.UpdatePlan(cfg.algorithm, actor, critic, log_alpha, target_critic, memory, actor_optimiser, critic_optimiser, temperature_optimiser, B, cfg.reinforcement.discount,
                         entropy_target, cfg.reinforcement.polyak_factor, expert_memory=expert_memory, discriminator=discriminator, discriminator_optimiser=discriminator_optimiser,
                         imitation_cfg=cfg.imitation if cfg.algorithm == 'GAIL' else None, mix_expert=mixed and cfg.algorithm in ('DRIL', 'GMMIL', 'RED'),
                         bc_aux=bool(cfg.imitation.bc_aux_loss))
  captured = False
  runner = plan
  if world > 1:
    if plan is None:
      raise NotImplementedError('distributed.world_size > 1 needs the captured update plan (a GAIL variant with per-update host inputs, or a batch size that is not a multiple of 16, has no data-parallel path)')
    runner = parallel.DataParallelUpdate(plan)   # grads-only kernels -> all-reduce(mean) of one flat bucket per sync point -> apply kernels

  # acting (train.py:151-168): il_act_step through a pinned mailbox. PWIL's per-step reward (models.py:216-249) is one more launch in front of the append, which stores it
  # from the device (ActingWorker(reward_model=...)): no compute_reward, and no reset() at episode ends - the coupling kernel sets the atom weights back itself
  schedule = (cfg.get('acting', {}) or {}).get('schedule', 'exact')  # `+acting.schedule=fused|overlap`: see imitation_learning_amd/acting.py (behaviour policy lags 1-2 updates)
  assert schedule in ('exact', 'fused', 'overlap', 'per_function')
  # general actor shapes (csrc/general.hip) take the same worker: one launch per step where the tile engine applies, else the layer-at-a-time launches + a commit kernel
  worker = None
  if schedule != 'per_function':
    try:
      worker = il.ActingWorker(actor, memory, mirror=schedule == 'overlap', reward_model=discriminator if cfg.algorithm == 'PWIL' else None)
    except NotImplementedError as e:   # overlap with an actor outside the one-launch shapes, PWIL atoms outside the one-launch coupling: the per-function path
      print(f'[train] +acting.schedule={schedule}: {e}; acting through the per-function path', file=sys.stderr)
  if worker is None: schedule = 'per_function'
  if schedule == 'overlap' and world > 1:
    raise NotImplementedError('+acting.schedule=overlap with distributed.world_size > 1: the overlap schedule captures the append in the update plan\'s hooks, which the '
                              'data-parallel runner does not run (use exact or fused)')
  if schedule == 'overlap' and plan is not None: worker.attach(plan)   # append + parameter snapshot ride in the update's hipGraph
  elif plan is not None: plan.main_feeds_ring = True   # appends are enqueued on this stream between updates: a resident index draw on the other stream must come after them
  if cfg.algorithm in ('GAIL', 'RED'): discriminator.eval()   # train.py:147: from here on the RED predictor's dropout is off (DRIL keeps its dropout on purpose)
  t, state, terminal, train_return = 0, env.reset(), False, 0
  action = worker.act(state) if schedule in ('fused', 'overlap') else None
  last_good = 0   # the last update step whose time-out words read zero (check_timeouts_seen)
  for step in range(1, cfg.steps + 1):
    if dog is not None: dog.beat(f'step {step}')
    update_due = step >= cfg.training.start and step % cfg.training.interval == 0
    if schedule == 'per_function':
      with torch.inference_mode():
        action = actor(state).sample()
        next_state, reward, terminal = env.step(action)
        t += 1
        reward_stored = discriminator.compute_reward(state, action) if cfg.algorithm == 'PWIL' else reward
        memory.append(step, state, action, reward_stored, next_state, terminal and t != env.max_episode_steps, t == env.max_episode_steps)
        if terminal and cfg.imitation.absorbing and t != env.max_episode_steps: memory.wrap_for_absorbing_states()
    else:
      if schedule == 'exact': action = worker.act(state)
      next_state, reward, terminal = env.step(action)
      t += 1
      timed_out = t == env.max_episode_steps
      following = env.reset() if terminal else next_state   # the observation the next action is for
      if schedule == 'exact':
        worker.append(step, next_state, reward, terminal and not timed_out, timed_out)
      elif schedule == 'fused':
        action = worker.step(step, next_state, reward, terminal and not timed_out, timed_out, obs=following)
      else:
        worker.post(step, state, action, next_state, reward, terminal and not timed_out, timed_out)
        if not (update_due and plan is not None):
          if plan is not None: plan.launcher_wait()   # (an update handed to the launcher thread is issued before this append)
          worker.enqueue_append()   # otherwise the update graph carries it
    train_return += reward
    if terminal:
      if cfg.algorithm == 'PWIL' and schedule == 'per_function': discriminator.reset()   # (through the worker the coupling launch of the episode's last transition has done it)
      metrics['train_steps'].append(step); metrics['train_returns'].append([train_return])
      t, train_return = 0, 0
      state = env.reset() if schedule == 'per_function' else following
    else:
      state = next_state

    act_early = schedule == 'overlap' and update_due and plan is not None and captured   # (round 6) the act launch ahead of the update's host work (ActingWorker.act_begin)
    if act_early: worker.act_begin(state)
    if update_due:
      if plan is not None:
        if cfg.algorithm == 'AdRIL': plan.relabel_args(step, memory.num_trajectories)   # the relabeller's per-update scalars -> device buffer (models.py:300-318)
        if not captured:
          runner.run()   # first update eagerly (loads code objects; GMMIL: fixes the kernel bandwidths), then capture
          if world > 1 and getattr(runner, 'handoff', False) and not runner.agree_on_handoff():   # collective decision (see DataParallelUpdate.agree_on_handoff)
            print(f'[train] rank {rank}: a bounded device-side wait expired during the first data-parallel update on some rank: every rank continues with stream dependencies '
                  '(the affected rank skipped that update - an expired wait poisons its learner -; every rank has been reset to rank 0\'s replica)', file=sys.stderr)
          if world > 1 and cfg.algorithm == 'GMMIL':   # one reward function on every rank: rank 0's bandwidths (models.py:193-195 freezes the first batch's)
            discriminator.gamma_1, discriminator.gamma_2 = parallel.broadcast_scalars([discriminator.gamma_1, discriminator.gamma_2])
          if world > 1 and cfg.distributed.backend != 'nccl' and getattr(runner, 'peer', None) is None:
            step_update = runner.run   # gloo collectives synchronise the host: not capturable (and a failed capture poisons the stream) - eager launches
          elif runner is plan and plan.direct_launch_ok() and os.environ.get('IL_TRAIN_LAUNCH', 'direct') != 'graph':
            # one GPU, the two-branch schedule: the update's six launches issued directly (two library calls per update). A hipGraph replay costs ~4.5 us more between
            # two updates than the launch boundary of the same kernels (profiles/r05_launch_ab.txt); IL_TRAIN_LAUNCH=graph keeps the graphs
            plan.record_direct()
            # (round 6) IL_TRAIN_LAUNCH_THREAD=1 with +acting.schedule=overlap: the recorded launches go out from the library's launcher thread (UpdatePlan.launch_async) while
            # this thread posts the next observation and steps the environment; every host-side read / launch of this learner below drains the launcher first. Opt-in: it pays
            # when an environment step costs more than the act launch's turn-around (a real simulator); on the synthetic environment it measured 10.3k against 11.5k
            # env-steps/s (profiles/r06_acting.json: the loop is bound by that turn-around, which then has nothing to hide behind).
            use_thread = schedule == 'overlap' and not plan._direct_overlap and not worker.general and os.environ.get('IL_TRAIN_LAUNCH_THREAD', '0') == '1'   # (il_act_step_general has more arguments than the launcher re-issues)
            step_update = plan.launch_async if use_thread else plan.launch_direct
          elif runner is not plan and runner.direct_launch_ok() and os.environ.get('IL_TRAIN_LAUNCH', 'direct') != 'graph':
            runner.record_direct()   # (round 6) data parallel with the exchanges inside the optimiser launches: the launch sequence of one GPU, issued the same way
            step_update = runner.launch_direct
          else:
            runner.capture(warmup=0)   # the gradient exchange (peer-window kernels, or RCCL collectives) is captured with the kernels: one graph replay per data-parallel update
            step_update = runner.replay
          captured = True
          plan.watch_timeouts(runner.peer.status if getattr(runner, 'peer', None) is not None else None)   # expired device-side waits raise a host-visible flag from now on
          if world > 1:   # graph capture takes different times on different ranks: meet again before the first replay, whose device-side waits are bounded
            torch.cuda.synchronize(); torch.distributed.barrier()
          if dog is not None: dog.arm(f'step {step}')
        else:
          step_update()
        check_timeouts_seen(plan, step, last_good)   # host read of pinned words: every step, independent of logging.interval
        last_good = step
        rewards, log_probs, Q_values = plan.transitions['rewards'], plan.logp, plan.q
      else:
        transitions, expert_transitions = memory.sample(B), expert_memory.sample(B)
        if cfg.algorithm == 'GAIL':
          discriminator.train()
          il.adversarial_imitation_update(actor, discriminator, transitions, expert_transitions, discriminator_optimiser, cfg.imitation)
          discriminator.eval()
        if cfg.imitation.mix_expert_data == 'mixed_batch' and cfg.algorithm in ('DRIL', 'GAIL', 'GMMIL', 'RED'):   # train.py:175,183: only inside the imitation block, never for SAC / PWIL / AdRIL
          il.mix_expert_agent_transitions(transitions, expert_transitions)
        if cfg.algorithm == 'AdRIL':
          discriminator.resample_and_relabel(transitions, expert_transitions, step, memory.num_trajectories, expert_memory.num_trajectories)
        if cfg.algorithm == 'GAIL':
          transitions['rewards'] = discriminator.predict_reward(**il.make_gail_input(transitions['states'], transitions['actions'], transitions['next_states'], transitions['terminals'], actor,
                                                                                     cfg.imitation.discriminator.reward_shaping, cfg.imitation.discriminator.subtract_log_policy))
        elif cfg.algorithm in ('DRIL', 'RED'):
          transitions['rewards'].copy_(discriminator.predict_reward(transitions['states'], transitions['actions']))
        elif cfg.algorithm == 'GMMIL':
          transitions['rewards'] = discriminator.predict_reward(transitions['states'], transitions['actions'], expert_transitions['states'], expert_transitions['actions'],
                                                                transitions['weights'].contiguous(), expert_transitions['weights'].contiguous())
        if cfg.imitation.bc_aux_loss: il.behavioural_cloning_update(actor, expert_transitions, actor_optimiser)
        log_probs, Q_values = il.sac_update(actor, critic, log_alpha, target_critic, transitions, actor_optimiser, critic_optimiser, temperature_optimiser, cfg.reinforcement.discount,
                                            entropy_target, cfg.reinforcement.polyak_factor)
        rewards = transitions['rewards']
      if schedule == 'overlap' and plan is None: worker.enqueue_publish()
      if cfg.logging.interval > 0 and step % cfg.logging.interval == 0:  # the only D2H reads of the update path (train.py:205-210)
        if plan is not None: plan.join()   # the logged tensors may have been written by the plan's second stream
        check_handoff(plan, step, runner)
        metrics['update_steps'].append(step); metrics['predicted_rewards'].append(rewards.cpu().numpy())
        metrics['alphas'].append(log_alpha.exp().cpu().numpy()); metrics['entropies'].append((-log_probs).cpu().numpy()); metrics['Q_values'].append(Q_values.cpu().numpy())

    if schedule == 'overlap': action = worker.act_end() if act_early else worker.act(state)   # own stream, published snapshot: returns while the update is still running

    if dog is not None and step % cfg.evaluation.interval == 0 and not cfg.check_time_usage:   # every rank: rank 0 evaluates, its peers wait for it inside their next collective
      dog.grace(0.005 * cfg.evaluation.episodes * env.max_episode_steps, 'evaluation')
    if step % cfg.evaluation.interval == 0 and not cfg.check_time_usage and lead:
      if plan is not None: plan.launcher_wait()
      episode_returns = evaluate()
      normalised = normalise(episode_returns)
      score.append(float(normalised.mean()))
      record_evaluation(cfg, metrics, file_prefix, step, episode_returns, normalised)
    if world > 1 and step % cfg.evaluation.interval == 0 and not cfg.check_time_usage:
      # rank 0 has just spent seconds evaluating: align the hosts here, so that no BOUNDED device-side wait of the next update (the peer-window exchange, the hand-off on
      # the all-reduced discriminator step) has to span that gap
      torch.cuda.synchronize(); torch.distributed.barrier()
      if plan is not None:   # replicas apply the same averaged gradients with the same kernels: anything but identical bits means an exchange went wrong - stop before training on
        check_handoff(plan, step, runner)
        same, digests = parallel.replicas_bit_identical(runner.replica_state())
        if not same:
          raise RuntimeError(f'step {step}: the data-parallel replicas are no longer bit-identical (sha256 per rank: {[d[:12] for d in digests]}; exchange: {runner.exchange_name()}). '
                             'Re-run with IL_PEER_EXCHANGE=0 (RCCL all-reduces).')
        metrics.setdefault('replica_checks', []).append((step, digests[0][:16], runner.exchange_name()))

  if plan is not None: plan.join()   # the discriminator is stepped on the plan's second stream: order the checkpoint reads after it
  check_handoff(plan, cfg.steps, runner)   # never save a learner whose last updates ran on expired device-side waits
  if world > 1:
    import torch.distributed as dist
    torch.cuda.synchronize(); dist.barrier()
    if plan is not None:
      same, digests = parallel.replicas_bit_identical(runner.replica_state())
      if not same:
        raise RuntimeError(f'end of training: the data-parallel replicas are not bit-identical (sha256 per rank: {[d[:12] for d in digests]}); nothing saved')
    dog.stop()
    if not lead:   # replicas are identical: rank 0 writes the checkpoint; the others return their (empty) score
      dist.destroy_process_group()
      return float('nan')
  if cfg.check_time_usage: metrics['training_time'] = time.time() - start_time
  save_run(cfg, file_prefix, metrics, actor, critic, log_alpha, discriminator, eval_env, lockstep)
  if world > 1:
    dist.destroy_process_group()
  return float(np.mean(score)) if score else float('nan')


# ---- seed sweeps (reference README.md:96-99: `python train.py -m seed=1,2,...`): the jobs of one sweep that differ only in their seed, as one population in one process
SWEEP_SCHEDULES = ('population', 'per_learner')
SWEEP_DEFAULT_SCHEDULE = 'per_learner'


def sweep_schedule(cfg) -> str:
  """`+sweep.schedule=population`: one il_act_step_population launch per lockstep environment step, the il_*_population launches per update, evaluate_population.
  `per_learner`: the same driver, learners, seeds and learner ids through one ActingWorker(noise_seed=seed) per learner, plan.run() per learner and evaluate_agent - the
  A/B partner, and the same bits."""
  schedule = (cfg.get('sweep', {}) or {}).get('schedule', SWEEP_DEFAULT_SCHEDULE)
  assert schedule in SWEEP_SCHEDULES, f'+sweep.schedule={schedule}: expected one of {SWEEP_SCHEDULES}'
  return schedule


PWIL_POPULATION_KEY = '+sweep.pwil_population=true'   # the opt-in of PWIL sweeps (`+sweep.schedule` alone keeps them job after job)
ADRIL_POPULATION_KEY = '+sweep.adril_population=true'   # the opt-in of AdRIL / SQIL sweeps (`+sweep.schedule` alone keeps them job after job)
GAIL_MIXUP_POPULATION_KEY = '+sweep.gail_mixup_population=true'   # the opt-in of GAIL sweeps whose loss is Mixup (without it they run job after job, whatever +sweep.schedule says)

# algorithm (Mixup: GAIL with that loss) -> (the key that opts its seed sweeps into a population, how that population trains): what sweep_fallback_reason appends while the
# key is missing. Each runs as it always has without its key; PWIL's, AdRIL's and Mixup's are keys of their own, which +sweep.schedule does not replace.
SWEEP_OPT_INS = {
    'DRIL': (f'+sweep.schedule={"|".join(SWEEP_SCHEDULES)}', 'DRIL trains as one population (il_dril_reward_population, il_bc_step_population)'),
    'PWIL': (PWIL_POPULATION_KEY, 'PWIL trains as one population (il_pwil_act_reward_population: one coupling launch per lockstep step)'),
    'AdRIL': (ADRIL_POPULATION_KEY, 'AdRIL trains as one population (il_batch_mix_relabel_population: one relabel launch per update)'),
    'Mixup': (GAIL_MIXUP_POPULATION_KEY, 'Mixup trains as one population (il_gail_mixup_step_population: every learner\'s coefficients under its own key and counter)'),
}


def sweep_opt_in(cfg, name: str) -> bool:
  """`+sweep.<name>=true` was given."""
  return bool((cfg.get('sweep', {}) or {}).get(name, False))


def gail_mixup_population(cfg) -> bool:   # the name tests/test_sweep_gail_mixup_config_cpu.py asks by
  return sweep_opt_in(cfg, 'gail_mixup_population')


def _opt_in_clause(which: str) -> str:
  key, how = SWEEP_OPT_INS[which]
  return f'; {how} only when {key} is given'


def pwil_atoms_upper_bound(cfg) -> tuple:
  """(most atoms a learner of this configuration can hold, horizon): kept trajectories x ceil(horizon / subsample) rows, plus - with absorbing states - the appended
  absorbing row and the two rows the subsampling always keeps (environments.dataset_to_memory). imitation.trajectories=0 keeps the whole dataset: counted as the synthetic
  stand-in's (+synthetic_env.dataset_trajectories, default 30); a larger real dataset is refused by the worker when it is built."""
  env_kw = dict(cfg.get('synthetic_env', {}) or {})
  horizon = int(env_kw.get('max_episode_steps', 1000))
  kept = int(cfg.imitation.trajectories) or int(env_kw.get('dataset_trajectories', 30))
  sub, absorbing = int(cfg.imitation.subsample), bool(cfg.imitation.absorbing)
  per_trajectory = -(-(horizon + int(absorbing)) // sub) + (2 if absorbing and sub > 1 else 0)
  return kept * per_trajectory, horizon


def _fused_shape(model_cfg) -> bool:
  return int(model_cfg.depth) == 2 and str(model_cfg.activation) == 'relu' and int(model_cfg.hidden_size) % 64 == 0 and 64 <= int(model_cfg.hidden_size) <= 256


def sweep_fallback_reason(cfg):
  """None when a seed sweep of this configuration can train as one population (what il.BatchedPopulationPlan and il.PopulationActingWorker take); otherwise the reason
  its jobs run one after another through train()."""
  explicit = (cfg.get('sweep', {}) or {}).get('schedule') is not None
  opted_in = {'DRIL': explicit, 'PWIL': sweep_opt_in(cfg, 'pwil_population'), 'AdRIL': sweep_opt_in(cfg, 'adril_population')}
  if cfg.algorithm not in ('SAC', 'GAIL', 'RED', 'GMMIL') and not opted_in.get(cfg.algorithm, False):
    reason = f'algorithm={cfg.algorithm} has no population launches (SAC, GAIL and RED have), and GMMIL under an explicit +sweep.schedule'
    return reason + (_opt_in_clause(cfg.algorithm) if cfg.algorithm in opted_in else '')
  if cfg.algorithm == 'GMMIL' and (cfg.get('sweep', {}) or {}).get('schedule') is None:
    # opt-in: a GMMIL sweep without the key runs as it always has; with it, its first update is eager (every learner's bandwidths) and the rest are population launches
    return f'algorithm=GMMIL trains as one population (il_gmmil_reward_population) only when +sweep.schedule={"|".join(SWEEP_SCHEDULES)} is given'
  if not (_fused_shape(cfg.reinforcement.actor) and _fused_shape(cfg.reinforcement.critic)):
    return 'an actor / critic shape outside depth 2, ReLU, hidden 64..256 in multiples of 64 has no population launches'
  if int(cfg.reinforcement.actor.hidden_size) != int(cfg.reinforcement.critic.hidden_size):
    return 'actor and critic of different hidden sizes have no population launches'
  if cfg.training.batch_size % 16 != 0:
    return f'training.batch_size={cfg.training.batch_size} is not a multiple of 16'
  # RED, GMMIL and DRIL with prefill_memory: the expert rows are moved into the agent ring once, in front of the loop (train.py:134, 192); nothing is edited between the launches
  # PWIL with prefill_memory: each learner relabels its expert memory on the device and moves it into its ring, once, in front of the loop (train.py:135-141, 192)
  # AdRIL's mixed_batch (config.validate demands it) is its relabel launch itself: il_batch_mix_relabel_population edits every learner's rows in ONE launch between the launches
  if cfg.imitation.mix_expert_data != 'none' and not (cfg.algorithm in ('RED', 'GMMIL', 'DRIL', 'PWIL') and cfg.imitation.mix_expert_data == 'prefill_memory') \
      and not (cfg.algorithm == 'AdRIL' and cfg.imitation.mix_expert_data == 'mixed_batch'):
    return f'imitation.mix_expert_data={cfg.imitation.mix_expert_data} edits the batches between the launches'
  if cfg.imitation.bc_aux_loss and cfg.algorithm != 'DRIL':   # DRIL (every shipped configuration sets it): il_bc_step_population in front of the forward launches
    return 'imitation.bc_aux_loss adds an actor step per update that the population launches do not have'
  if int(cfg.distributed.world_size) != 1:
    return 'distributed.world_size > 1: a population is a single-GPU mode'
  acting = (cfg.get('acting', {}) or {}).get('schedule', 'exact')
  if acting not in ('exact', 'fused'):
    return f'+acting.schedule={acting}: the population acting launch has the exact and the fused schedule'
  if cfg.algorithm == 'PWIL':
    n, horizon = pwil_atoms_upper_bound(cfg)
    m, chunks = int(np.ceil((1 / horizon - 1e-6) * n)) + 2, -(-n // 256)
    if m > 256 or chunks * m > 4096:
      return (f'PWIL with up to {n} atoms at horizon {horizon} lies outside the one-launch coupling il_pwil_act_reward_population runs per learner: it needs m = ceil(N / T) + 2 <= 256 '
              f'consumable atoms per step and ceil(N / 256) * m <= 4096 candidates (here m = {m}, {chunks} chunks)')
  if cfg.algorithm == 'GMMIL':
    S, A = env_dims(cfg.env, cfg.imitation.absorbing)
    D = S + (0 if cfg.imitation.state_only else A)
    if D > 128:
      return f'GMMIL on {D} state + action dims: above 128 the reward runs its direct-difference launches per learner (il_gmmil_reward_population covers dims <= 128)'
  if cfg.algorithm == 'GAIL':
    d = cfg.imitation.discriminator
    if (int(d.depth), str(d.activation)) != (1, 'relu'):
      return 'a depth-2 / tanh discriminator runs its per-function entry points inside the plan'
    if d.reward_shaping or d.subtract_log_policy:
      return 'reward shaping / subtract_log_policy run their per-function entry points inside the plan'
    if cfg.imitation.loss_function == 'PUGAIL' and float(cfg.imitation.nonnegative_margin) != float('inf'):
      return 'a finite PUGAIL margin needs a value pass ahead of the gradients'
    if cfg.imitation.loss_function == 'Mixup' and not sweep_opt_in(cfg, 'gail_mixup_population'):   # at any mixup_alpha
      return 'imitation.loss_function=Mixup has no population discriminator step (BCE and PUGAIL with an infinite margin have)' + _opt_in_clause('Mixup')
  return None


def _without_seed(cfg, also=()) -> dict:
  import copy
  d = copy.deepcopy(dict(cfg))
  d.pop('seed', None)
  for k in also: d.pop(k, None)
  return d


def sweep_groups(cfgs):
  """The jobs of a sweep as runs: [(job numbers, reason)] in job order. reason None: those jobs differ only in `seed` and train as one population (train_sweep);
  otherwise a single job for train(), with the reason it is not part of a population."""
  keys, members = [], []
  for j, cfg in enumerate(cfgs):
    k = _without_seed(cfg)
    for i, other in enumerate(keys):
      if other == k:
        members[i].append(j); break
    else:
      keys.append(k); members.append([j])
  runs = []
  for jobs in members:
    reason = sweep_fallback_reason(cfgs[jobs[0]])
    if reason is None and len(jobs) == 1:
      reason = 'no other job of the sweep differs from it in the seed alone'
    if reason is None and len({cfgs[j].seed for j in jobs}) != len(jobs):
      reason = 'two jobs with the same seed'
    runs += [(jobs, None)] if reason is None else [([j], reason) for j in jobs]
  return sorted(runs, key=lambda r: r[0][0])


def sweep_dir(cfg, stamp: str) -> str:
  """The reference's hydra.sweep.dir: outputs/${algorithm}_${env}_sweeper/<time>; job n writes into its subdirectory n."""
  return os.path.join('outputs', f'{cfg.algorithm}_{cfg.env}_sweeper', stamp)


def mixed_env_fallback_reason(cfg):
  """None when learners of this configuration on DIFFERENT environments (train_all.py: different state / action widths) can train as one population; otherwise why not.
  The population launches serve learners of different widths for SAC and for GAIL without Mixup (the `_mixed` entry points of include/il_hip.h)."""
  reason = sweep_fallback_reason(cfg)
  if reason is not None: return reason
  if cfg.algorithm not in ('SAC', 'GAIL'):
    return f'algorithm={cfg.algorithm} has no population launches for learners of different state / action widths (SAC and GAIL have)'
  if cfg.algorithm == 'GAIL' and cfg.imitation.loss_function == 'Mixup':
    return 'imitation.loss_function=Mixup has no population discriminator step for learners of different state / action widths'
  return None


def train_sweep(cfgs, prefixes, vary_env: bool = False, noise_ids=None):
  """`vary_env` (train_all.py): the learners may also differ in `env`, i.e. in their state / action widths - SAC and GAIL without Mixup (mixed_env_fallback_reason).
  `noise_ids` (train_all.py -m): per learner, the id its Philox key is derived from instead of its position in the population - a job's four learners then draw the noise
  they draw when that job runs alone, wherever they stand in a population of several jobs. The key is seed + 7919 * (id + 1), as for positions: two learners of one population
  share a key only if their seeds differ by a multiple of 7919 on different ids (seed=3 on id 1 and seed=7922 on id 0) - different environments then, so different streams of use.
  The loop of train() in lockstep over L learners that differ only in their seed: per lockstep step ONE population act launch, L host environment steps and ONE
  append launch (`+acting.schedule=fused`: one launch for both); on update steps ONE population update (il.BatchedPopulationPlan); on evaluation steps
  evaluate_population. Every learner has its own seeds, index stream, environments, rings, networks, optimisers and `learner_id`; job l writes what a single run writes
  under prefixes[l] (GAIL, RED and DRIL: with a discriminator.pth; PWIL, AdRIL and GMMIL, as in train(): without one - its bandwidths are fixed by each learner's first batch, in the first, eager,
  update, and live in no file). Returns the mean normalised score per job."""
  L = len(cfgs)
  assert L >= 1 and len(prefixes) == L
  for cfg in cfgs: il_config.validate(cfg)
  cfg0 = cfgs[0]
  if vary_env:
    assert all(_without_seed(c, ('env',)) == _without_seed(cfg0, ('env',)) for c in cfgs), 'train_sweep: the jobs of one population differ only in seed and env'
  else:
    assert all(_without_seed(c) == _without_seed(cfg0) for c in cfgs), 'train_sweep: the jobs of one population differ only in their seed'
  for c in (cfgs if vary_env else cfgs[:1]):
    reason = mixed_env_fallback_reason(c) if vary_env and len({x.env for x in cfgs}) > 1 else sweep_fallback_reason(c)
    if reason is not None: raise NotImplementedError(f'train_sweep: {reason}')
  how, schedule = sweep_schedule(cfg0), (cfg0.get('acting', {}) or {}).get('schedule', 'exact')
  evaluation_schedule(cfg0)
  dev = default_device()
  assert _lib.on_device(torch.empty(0, device=dev)), 'train.py needs a GPU: the update path has no CPU fallback'
  B, env_kw = cfg0.training.batch_size, dict(cfg0.get('synthetic_env', {}) or {})
  mixup_sweep = cfg0.algorithm == 'GAIL' and cfg0.imitation.loss_function == 'Mixup'   # (sweep_fallback_reason: under +sweep.gail_mixup_population=true only)
  start_time = time.time()   # check_time_usage: training_time is what train() reports - everything after the environments, the expert data and the networks are built

  learners = []
  for i, cfg in enumerate(cfgs):
    ln = _Learner()
    ln.cfg, ln.prefix, seed, built = cfg, prefixes[i], cfg.seed, time.time()
    il.seed(seed); np.random.seed(seed); torch.manual_seed(seed)   # in front of this learner's construction: its data, initialisation and pretraining are its seed's
    ln.stream = il.IndexStream(seed)   # the learner's own replay index stream (agent batch, then expert batch, per update)
    ln.env, ln.eval_env = make_env(cfg.env, cfg.imitation.absorbing, load_data=True, **env_kw), make_env(cfg.env, cfg.imitation.absorbing, **env_kw)
    ln.env.seed(seed); ln.eval_env.seed(seed)
    lo, hi = ln.env.env.ref_min_score, ln.env.env.ref_max_score
    ln.normalise = lambda returns, lo=lo, hi=hi: (np.asarray(returns) - lo) / (hi - lo)
    ln.expert_memory = ln.env.get_dataset(trajectories=cfg.imitation.trajectories, subsample=cfg.imitation.subsample, device=dev)
    S, A = ln.env.observation_space.shape[0], ln.env.action_space.shape[0]
    build_agent(ln, cfg, S, A, dev)
    ln.memory.index_rng = ln.expert_memory.index_rng = ln.stream
    ln.discriminator, ln.discriminator_optimiser = build_reward_model(cfg, S, A, ln.expert_memory, ln.env.max_episode_steps)
    ln.metrics, ln.score = new_metrics(), []
    start_time += time.time() - built
    began = time.time()
    if cfg.bc_pretraining.iterations > 0:
      pretrain_bc(cfg, ln.actor, ln.expert_memory, S, A)   # one PretrainPlan per learner
    if cfg.algorithm in ('DRIL', 'RED'):   # train.py:114-134 in train()'s order, under this learner's seeds: pretraining, its own threshold / bandwidth, the prefill
      pretrain_reward_model(cfg, ln.discriminator, ln.discriminator_optimiser, ln.expert_memory, S, A)
      if cfg.check_time_usage:   # what train() reports: this learner's pretraining on its own, and a training_time that starts behind it
        ln.metrics['pre_training_time'] = time.time() - began
        start_time += ln.metrics['pre_training_time']
      if cfg.imitation.mix_expert_data == 'prefill_memory': ln.memory.transfer_transitions(ln.expert_memory)
      if cfg.algorithm == 'RED': ln.discriminator.eval()   # train.py:147, in front of the plan: from here on the predictor's dropout is off
    if cfg.algorithm == 'GMMIL' and cfg.imitation.mix_expert_data == 'prefill_memory': ln.memory.transfer_transitions(ln.expert_memory)   # train.py:192, once, in front of the loop
    if cfg.algorithm == 'PWIL' and cfg.imitation.mix_expert_data == 'prefill_memory':   # train.py:135-141, 192 as train() runs them: the relabel on the device (or row by row), then the prefill
      if pretraining_schedule(cfg) == 'plan':
        ln.discriminator.relabel_memory(ln.expert_memory)   # (sweep_fallback_reason has bounded the atoms: inside the one-launch coupling)
      else:
        relabel_row_by_row(ln.discriminator, ln.expert_memory)
      ln.memory.transfer_transitions(ln.expert_memory)
    ln.plan = il.UpdatePlan(cfg.algorithm, ln.actor, ln.critic, ln.log_alpha, ln.target_critic, ln.memory, ln.actor_optimiser, ln.critic_optimiser, ln.temperature_optimiser, B,
                            cfg.reinforcement.discount, ln.entropy_target, cfg.reinforcement.polyak_factor, expert_memory=ln.expert_memory, discriminator=ln.discriminator,
                            discriminator_optimiser=ln.discriminator_optimiser, imitation_cfg=cfg.imitation if cfg.algorithm == 'GAIL' else None, overlap=False, learner_id=i,
                            bc_aux=bool(cfg.imitation.bc_aux_loss),   # (sweep_fallback_reason: set for DRIL learners only)
                            noise_seed_offset=0 if cfg.algorithm == 'PWIL' or mixup_sweep else (None if noise_ids is None else 7919 * (int(noise_ids[i]) + 1)))   # PWIL and Mixup jobs train as train() trains them, bit for bit: its Philox key for this learner's seed
    ln.plan.main_feeds_ring = True
    ln.plan.watch_timeouts()
    if ln.discriminator is not None and cfg.algorithm not in ('DRIL', 'PWIL', 'AdRIL'): ln.discriminator.eval()   # train.py:147 (the DRIL ensemble keeps its dropout, i.e. train mode, on purpose)
    learners.append(ln)
  plans = [ln.plan for ln in learners]

  # +evaluation.schedule=lockstep: E seeded evaluation environments per learner; under the population schedule ONE evaluator (one launch per lockstep step for all L x E
  # rows), under per_learner one evaluator per learner - per row the same action either way, so the same bytes
  lock_all, lock_own = None, None
  if how == 'population': lock_all = lockstep_evaluator(cfg0, [ln.actor for ln in learners])
  else: lock_own = lockstep_evaluator(cfg0, [ln.actor for ln in learners], each=True)
  for ln in learners:
    ln.eval_envs = lockstep_eval_envs(ln.cfg, ln.cfg.seed, ln.eval_env, env_kw) if lock_all is not None or lock_own is not None else None

  if how == 'population':
    pop = il.BatchedPopulationPlan(plans)
    # PWIL: every learner's coupling in ONE launch ahead of the population acting launch; the rewards are stored from the device, and the kernel resets the atom weights at episode ends
    worker = il.PopulationActingWorker([ln.actor for ln in learners], [ln.memory for ln in learners], [ln.cfg.seed for ln in learners],
                                       reward_models=[ln.discriminator for ln in learners] if cfg0.algorithm == 'PWIL' else None)
    update = pop.run
  else:
    pop, worker = None, None
    workers = [il.ActingWorker(ln.actor, ln.memory, noise_seed=ln.cfg.seed, reward_model=ln.discriminator if cfg0.algorithm == 'PWIL' else None) for ln in learners]
    def update():
      for p in plans: p.run()

  every = range(L)
  widths = [ln.env.action_space.shape[0] for ln in learners]   # learner l's own action components: row l of the population's [L, widest A] tensor, or its own worker's [1, A_l]
  own = lambda action, l: action[l] if isinstance(action, list) else action[l:l + 1, :widths[l]]
  t, train_return = [0] * L, [0.0] * L
  state = [ln.env.reset() for ln in learners]
  action = None
  if schedule == 'fused':
    action = worker.act(state) if worker is not None else [workers[l].act(state[l]) for l in every]
  captured, last_good = False, 0
  for step in range(1, cfg0.steps + 1):
    if schedule == 'exact':
      action = worker.act(state) if worker is not None else [workers[l].act(state[l]) for l in every]
    next_state, reward, terminal, timed_out, following = [None] * L, [0.0] * L, [False] * L, [False] * L, [None] * L
    for l, ln in enumerate(learners):
      next_state[l], reward[l], terminal[l] = ln.env.step(own(action, l))
      t[l] += 1
      timed_out[l] = t[l] == ln.env.max_episode_steps
      following[l] = ln.env.reset() if terminal[l] else next_state[l]   # the observation the next action is for
    true_terminal = [terminal[l] and not timed_out[l] for l in every]
    if schedule == 'exact':
      if worker is not None: worker.append(step, next_state, reward, true_terminal, timed_out)
      else:
        for l in every: workers[l].append(step, next_state[l], reward[l], true_terminal[l], timed_out[l])
    else:
      if worker is not None: action = worker.step(step, next_state, reward, true_terminal, timed_out, obs=following)
      else: action = [workers[l].step(step, next_state[l], reward[l], true_terminal[l], timed_out[l], obs=following[l]) for l in every]
    for l, ln in enumerate(learners):
      train_return[l] += reward[l]
      if terminal[l]:
        ln.metrics['train_steps'].append(step); ln.metrics['train_returns'].append([train_return[l]])
        t[l], train_return[l] = 0, 0.0
      state[l] = following[l]

    if step >= cfg0.training.start and step % cfg0.training.interval == 0:
      if cfg0.algorithm == 'AdRIL':   # models.py:300-318: every learner's {n_expert, round, policy trajectories} of this update, in front of its run or replay
        if pop is not None: pop.relabel_args(step, [ln.memory.num_trajectories for ln in learners])   # one stream-ordered copy of the 3 L words
        else:
          for ln in learners: ln.plan.relabel_args(step, ln.memory.num_trajectories)
      if pop is not None and captured:
        pop.replay()
      else:
        update()
        if pop is not None and not captured and os.environ.get('IL_TRAIN_LAUNCH', 'direct') == 'graph':   # the first update eagerly (loads the code objects), then one replay per update
          pop.capture(warmup=0)
          captured = True
      for p in plans: check_timeouts_seen(p, step, last_good)   # host reads of pinned words: every step, independent of logging.interval
      last_good = step
      if cfg0.logging.interval > 0 and step % cfg0.logging.interval == 0:  # the only D2H reads of the update path (train.py:205-210)
        for ln in learners:
          p, m = ln.plan, ln.metrics
          p.join()
          check_handoff(p, step)
          m['update_steps'].append(step); m['predicted_rewards'].append(p.transitions['rewards'].cpu().numpy())
          m['alphas'].append(ln.log_alpha.exp().cpu().numpy()); m['entropies'].append((-p.logp).cpu().numpy()); m['Q_values'].append(p.q.cpu().numpy())

    if step % cfg0.evaluation.interval == 0 and not cfg0.check_time_usage:
      if lock_all is not None:
        returns = evaluate_population_lockstep(lock_all, [ln.eval_envs for ln in learners], cfg0.evaluation.episodes)
      elif lock_own is not None:
        returns = [evaluate_agent_lockstep(ln.actor, ln.eval_envs, cfg0.evaluation.episodes, evaluator=e) for ln, e in zip(learners, lock_own)]
      elif worker is not None:
        returns = evaluate_population(worker, [ln.eval_env for ln in learners], cfg0.evaluation.episodes)
      else:
        returns = [evaluate_agent(ln.actor, ln.eval_env, cfg0.evaluation.episodes) for ln in learners]
      for ln, episode_returns in zip(learners, returns):
        normalised = ln.normalise(episode_returns)
        ln.score.append(float(normalised.mean()))
        record_evaluation(ln.cfg, ln.metrics, ln.prefix, step, episode_returns, normalised)

  for p in plans:   # never save a learner whose last updates ran on expired device-side waits
    p.join()
    check_timeouts_seen(p, cfg0.steps, last_good)
    check_handoff(p, cfg0.steps)
  torch.cuda.synchronize()
  scores = []
  for ln in learners:
    cfg, m = ln.cfg, ln.metrics
    if cfg.check_time_usage: m['training_time'] = time.time() - start_time
    lockstep = None
    if lock_all is not None and cfg.save_trajectories: lockstep = (il.LockstepEvaluator([ln.actor], max(int(cfg.evaluation.episodes), 1)), ln.eval_envs)   # one learner's final pass: an evaluator of its own
    elif lock_own is not None: lockstep = (lock_own[learners.index(ln)], ln.eval_envs)
    save_run(cfg, ln.prefix, m, ln.actor, ln.critic, ln.log_alpha, ln.discriminator, ln.eval_env, lockstep)
    scores.append(float(np.mean(ln.score)) if ln.score else float('nan'))
  return scores


def multirun(argv, stamp=None):
  """`python train.py -m ...`: compose the jobs, group them, run every group. Returns (sweep directory, scores in job order)."""
  cfgs, overrides = il_config.compose_multirun(argv)
  root = os.path.abspath(sweep_dir(cfgs[0], stamp or time.strftime('%m-%d_%H-%M-%S')))
  prefixes = []
  for j in range(len(cfgs)):
    os.makedirs(os.path.join(root, str(j)), exist_ok=True)
    prefixes.append(os.path.join(root, str(j), ''))
  scores = [None] * len(cfgs)
  for jobs, reason in sweep_groups(cfgs):
    if reason is None:
      print(f'[train] sweep: jobs {jobs[0]}..{jobs[-1]} ({" | ".join(" ".join(overrides[j]) for j in jobs)}) train as one population of {len(jobs)} learners '
            f'(+sweep.schedule={sweep_schedule(cfgs[jobs[0]])}'
            + (f', {GAIL_MIXUP_POPULATION_KEY}: il_gail_mixup_step_population at mixup_alpha={cfgs[jobs[0]].imitation.mixup_alpha}'
               if cfgs[jobs[0]].algorithm == 'GAIL' and cfgs[jobs[0]].imitation.loss_function == 'Mixup' else '') + ')', file=sys.stderr)
      for j, sc in zip(jobs, train_sweep([cfgs[j] for j in jobs], [prefixes[j] for j in jobs])): scores[j] = sc
    else:
      j = jobs[0]
      print(f'[train] sweep: job {j} ({" ".join(overrides[j])}) runs on its own, one job after another: {reason}', file=sys.stderr)
      scores[j] = train(cfgs[j], file_prefix=prefixes[j])
  for j, cfg in enumerate(cfgs):
    print(f'#{j} {" ".join(overrides[j])}: {cfg.algorithm} {cfg.env}: mean normalised score {scores[j]:.4f} (outputs in {os.path.join(root, str(j))})')
  return root, scores


def main(argv):
  if any(o in ('-m', '--multirun') for o in argv):
    return multirun(argv)[1]
  cfg = il_config.compose(argv)
  out = os.path.join('outputs', f'{cfg.algorithm}_{cfg.env}', time.strftime('%m-%d_%H-%M-%S'))
  if int(os.environ.get('RANK', '0')) == 0:   # data-parallel runs: rank 0 owns the output directory (the other ranks write nothing)
    os.makedirs(out, exist_ok=True)
    os.chdir(out)  # hydra.job.chdir=true in the reference
  score = train(cfg)
  print(f'{cfg.algorithm} {cfg.env}: mean normalised score {score:.4f} (outputs in {out})')
  return score


if __name__ == '__main__':
  main(sys.argv[1:])
