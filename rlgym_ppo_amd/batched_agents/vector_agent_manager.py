"""Rollout collection for ONE vectorised environment that steps all of its agents in lockstep, with the rollout kept on
the GPU (device-resident rollout storage, vector-env fast path).

The reference collects through one OS process per environment, a UDP datagram per step and Python lists per agent
(batched_agent_manager.py:126-299, batched_trajectory.py:58-105); at 4096 agents that is 4096 datagrams per step and,
per iteration, seven `np.asarray` flattens plus a 224 MB upload of the states.  Here the policy's padded input rows of
step t are written straight into their final, trajectory-major position on the device (row a*T + t of agent a), so
`Learner.add_new_experience` runs the value pass, the GAE scan and the buffer submit on them without a copy through the host.

What comes out is exactly what the reference's assembler would produce for the same interaction sequence when every agent
is its own trajectory stream (tests/test_gpu_vector_rollout.py compares with a numpy restatement of these rules):
  * trajectories are concatenated agent by agent, steps in order (batched_trajectory.py:58-105);
  * the last collected step of every agent is force-marked truncated unless it is terminal (quirk Q4, the flush at
    batched_agent_manager.py:154-172), and the episode continues in the next collect;
  * observations are standardised with the SCALAR statistics of feature 0 and clipped to +-5 (quirk Q5, :303-315), the
    running statistics are advanced every `steps_per_obs_stats_increment` steps with the raw observations (:233-235);
  * `next_states[i]` is the observation the environment returned for step i (after its auto-reset at episode ends).

Environment interface: `reset() -> obs [n, d]`; `step(actions [n, k]) -> (obs [n, d], rewards [n], dones [n],
truncated [n], info)` with auto-reset of finished agents; `observation_space.shape`, `action_space` as in the reference.
Optional (the sb3-contrib convention; discrete and multi-discrete policies): `action_masks() -> [n, n_actions]` booleans for the
observation the agents act on next ([n, sum(bins)] for a multi-discrete policy: one entry per bin of every component), called
after `reset()` and after every `step()`; the policy then samples valid actions only and the masks leave the collect
trajectory-major as `self.action_mask_rows` (next to `value_input_rows`).
Optional, asked for with `critic_observations` (Learner(critic_observations=True)) only: `critic_observations() -> [n, d_c]`, the
critic's own ("privileged") observation of the state the agents act on next, called after `reset()` and after every `step()` like
`action_masks()` (a device environment answers a device tensor).  The rows are standardised by a second running statistic,
`critic_obs_stats` (same cadence, same per-feature flag, first collect raw), staged with the critic's arena and leave the collect
trajectory-major as `self.critic_value_input_rows`, [N + 1, ld_c] next to `value_input_rows`: what the value pass and the buffer's
`critic_states` read.  The 7-tuple of `collect_timesteps` is what it was.
Optional, used with `bootstrap_truncated` (Learner(gae_bootstrap_truncated=True)) only: `info["final_observation"]`, float
[n, d], whose rows are meaningful where `truncated` is set and `done` is not -- the observation the episode ended on, which
the auto-reset has replaced in `obs`.  Those rows are standardised like that step's `obs`, kept out of the running
statistics and put into the next-state rows of those steps; the collect then leaves `bootstrap_steps`, `bootstrap_index`
and `bootstrap_rows` (the truncated-and-not-done steps and their next-state rows) for the GAE scan.

Device interface (an environment that itself lives on the GPU; chosen when `reset()` answers a torch.Tensor on a GPU, collected by
`_collect_device`; a numpy environment takes the two host forms exactly as they are):
  * `reset() -> Tensor[n, d]`, float32 or float64;
  * `step(actions) -> (obs[n, d], rewards[n], dones[n], truncated[n], info)`, or the 4-tuple without `truncated`: `actions` is a
    fresh float32 device tensor [n, k] in the host interface's float encoding, never a view of the rollout storage; `rewards`
    float32 or float64, the flags bool, uint8 or float (zero / non-zero);
  * the environment works on torch's current stream and may reuse its output tensors at the next `step`: the manager has consumed
    them by then in stream order;
  * optional `action_masks() -> bool Tensor[n, width]` on the device, packed by `Layout.pack`'s device branch (nothing is read back;
    an empty row counts as all-valid, as documented there);
  * optional `info["final_observation"]`, Tensor[n, d], with `bootstrap_truncated`: staged with that step's standardisation vectors
    and put into the next-state rows where the environment truncated and did not terminate.  The host does not know which steps
    those are: the collect leaves the DENSE form, `bootstrap_dense = True` and `bootstrap_rows` = all N next-state rows (the scan
    selects by the flags);
  * `info["state"]` and `collect_metrics_fn` as above; a metrics function that reads the device is the user's own wait.
Within a collect the host enqueues work and never waits for the device; it reads back once, at the end (the observation statistics,
the reward average and the ended-episode count in one copy).  An environment on another GPU than the policy's is a ValueError.
"""
import time
import warnings

import numpy as np
import torch

from ..util import action_mask as AM
from ..util.running_stats import WelfordRunningStat
from .batched_agent import describe_action_space


def device_env_of(first_obs):
    """Which interface an environment speaks, judged by what its reset() answered: the torch.device of a tensor on a GPU (the device
    interface, _collect_device), or None (numpy arrays, lists, CPU tensors: the host interface)."""
    if isinstance(first_obs, torch.Tensor) and first_obs.is_cuda:
        return first_obs.device
    return None


def check_same_device(env_device, policy_device):
    """A device environment must live on the policy's GPU: the collect enqueues both on one stream."""
    env_device, policy_device = torch.device(env_device), torch.device(policy_device)
    same = env_device.type == policy_device.type and (env_device.index is None or policy_device.index is None
                                                      or env_device.index == policy_device.index)
    if not same:
        raise ValueError(f"the vector environment lives on {env_device} but the policy on {policy_device}: a device-resident "
                         "environment must be on the policy's device")


_DT_CODES = {torch.float32: 0, torch.float64: 1, torch.bool: 2, torch.uint8: 2}   # RLPPO_DT_*


def _dt_code(x, what, device, n):
    """Device array of one step (rewards / flags) -> (tensor the record kernel reads, dtype code)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"a device-resident vector environment answers device tensors: step() returned {what} as "
                         f"{type(x).__name__}" + (f" on {x.device}" if isinstance(x, torch.Tensor) else ""))
    check_same_device(x.device, device)
    x = x.detach().reshape(-1)
    if x.numel() != n:
        raise ValueError(f"step() returned {x.numel()} {what} for {n} agents")
    if x.dtype not in _DT_CODES:
        x = x.to(torch.float32)
    return x.contiguous(), _DT_CODES[x.dtype]


class _HostInterfaceGuard(object):
    """An environment whose reset() answered a CPU tensor speaks the host interface; a step() that then answers device tensors is
    refused by name (numpy would fail on them with a conversion error)."""

    def __init__(self, env):
        self._env = env

    def step(self, actions):
        out = self._env.step(actions)
        if isinstance(out[0], torch.Tensor) and out[0].is_cuda:
            raise ValueError(f"the vector environment's reset() returned a CPU tensor but its step() returns observations on "
                             f"{out[0].device}: a device-resident environment answers device tensors from reset() on")
        return out

    def __getattr__(self, name):
        if name.startswith("__") or name == "_env":
            raise AttributeError(name)
        return getattr(self._env, name)


class _DeviceBook(object):
    """What _collect_device keeps on the device between environment steps, one allocation read back in ONE copy per collect:
    blob = [ state: int64[3] = bits of the double episode-reward average, has-value word, ended-episode counter |
             mean[d] | m2[d] : the running observation statistics in the host state's dtype (float32; float64 after a checkpoint load) ],
    ep_sums double[n]; two pairs of standardisation vectors (mean_v, std_v): a step's increment writes the pair that the
    observations still waiting for the previous pair do not read."""

    def __init__(self, device, n_agents):
        self.device, self.d, self.f64 = device, -1, False
        self.ep_sums = torch.zeros(n_agents, dtype=torch.float64, device=device)
        self.blob = self.pin = self.state = self.mean = self.m2 = None
        self.vec, self.cur = None, 0

    def layout(self, d, f64):
        if self.blob is not None and (d, f64) == (self.d, self.f64):
            return
        self.d, self.f64 = d, f64
        es, dt = (8, torch.float64) if f64 else (4, torch.float32)
        size = 24 + 2 * d * es
        self.blob = torch.zeros(size, dtype=torch.uint8, device=self.device)
        self.pin = torch.zeros(size, dtype=torch.uint8, pin_memory=True)
        self.state = self.blob[:24].view(torch.int64)
        self.mean = self.blob[24:24 + d * es].view(dt)
        self.m2 = self.blob[24 + d * es:].view(dt)
        if d and self.vec is None:
            self.vec = [tuple(torch.empty(d, dtype=torch.float32, device=self.device) for _ in range(2)) for _ in range(2)]


class VectorAgentManager(object):
    def __init__(self, policy, min_inference_size=8, seed=123, standardize_obs=True, steps_per_obs_stats_increment=5):
        self.policy = policy
        self.seed = seed
        self.standardize_obs = standardize_obs
        self.steps_per_obs_stats_increment = steps_per_obs_stats_increment
        self.steps_since_obs_stats_update = 0
        self.per_feature_obs_standardization = False  # True: every feature with its own statistics (not the reference's Q5)
        self.obs_stats = None
        self.cumulative_timesteps = 0
        self.average_reward = None
        self.env = None
        self.collect_metrics_fn = None
        self.n_agents = 0
        self.value_input_rows = None  # [N + 1, ld] device rows of the last collect: states ++ the last next_state
        self._next_rows = None        # padded device rows of the observation the agents act on next
        self._pending_obs = None      # fused collect: (raw device observations, standardisation scalars) the agents act on next
        self._ep_rews = None
        self.action_mask_rows = None  # util.action_mask.Packed [N, W] of the last collect (trajectory-major), or None: env without masks
        self._pending_mask = None     # packed device words [n_agents, W] of the observation the agents act on next
        # Learner(gae_bootstrap_truncated=True): every collect leaves what the bootstrap form of the GAE scan needs; off, a collect
        # does exactly what it did without the option
        self.bootstrap_truncated = False
        self.bootstrap_steps = None   # int64 host indices (trajectory-major) of the steps with truncated and not done
        self.bootstrap_index = None   # the same on the device; None when they are exactly the last step of every agent (the flush)
        self.bootstrap_rows = None    # [m, ld] device rows: the next states of those steps, in the order of bootstrap_steps
        self.bootstrap_dense = False  # True (device environment): bootstrap_rows are ALL N next-state rows, the scan selects by the flags
        self._warned_no_final_obs = False
        self._env_device = None       # torch.device of a device-resident environment (its reset() answered a GPU tensor), else None
        self._book = None             # _DeviceBook: the device environment's persistent bookkeeping
        self.last_enqueue_seconds = None   # device environment: host seconds the last collect spent enqueuing, before its one read
        self.episodes_ended = 0       # device environment: episodes ended so far (read back with the average at the end of a collect)
        # Learner(critic_observations=True): the critic's own observation rows (module docstring); off, a collect does what it did
        self.critic_observations = False
        self.value_net = None                  # the critic (its arena stages the rows); set by Learner once it exists
        self.critic_obs_size = None            # d_c, from the environment's first answer
        self.critic_obs_stats = None           # WelfordRunningStat(d_c), moved when obs_stats moves
        self.critic_value_input_rows = None    # [N + 1, ld_c] device rows of the last collect, mirroring value_input_rows
        self._critic_initial = None            # the answer after reset(): acted on RAW by the first collect
        self._critic_next_rows = None          # [n_agents, ld_c] staged rows of the observation the agents act on next
        self._cbook = None                     # _DeviceBook of critic_obs_stats (device environment)

    def _env_mask(self):
        """The environment's action_masks() for the observation the agents act on next, packed on the device; None without it."""
        fn = getattr(self.env, "action_masks", None)
        if fn is None:
            return None
        lay = AM.Layout.of(self.policy)
        m = np.asarray(fn())
        if m.ndim == 1:   # a one-agent environment may answer [n_actions]
            m = m.reshape(1, -1)
        if m.ndim != 2 or m.shape[1] != lay.width:
            raise ValueError(f"the environment's action_masks() has shape {tuple(m.shape)}: its width must be {lay.width}, the policy's "
                             + ("logit count sum(bins) (one entry per bin of every component)" if lay.heads is not None else "action count"))
        return lay.pack(m, self.policy.arena.device)

    def _masks_out(self, M, na, T):
        """Time-major words [T, na, W] -> self.action_mask_rows, trajectory-major (row a * T + t)."""
        self.action_mask_rows = None if M is None else AM.Packed(M.transpose(0, 1).reshape(na * T, M.shape[2]).contiguous(),
                                                                 AM.Layout.of(self.policy).width)

    @property
    def action_masks(self):
        """bool [N, n_actions] of the last collect, trajectory-major; None when the environment has no action_masks()."""
        return None if self.action_mask_rows is None else self.action_mask_rows.unpack()

    # --------------------------------------------------------------------------------------- critic observations
    def _critic_answer(self, dev=None):
        """The environment's critic_observations() for the observation the agents act on next: host interface -> float32 numpy
        [n_agents, d_c]; device interface (dev given) -> float32 device tensor."""
        x = self.env.critic_observations()
        if dev is not None or self._env_device is not None:
            if not (isinstance(x, torch.Tensor) and x.is_cuda):
                raise ValueError("a device-resident vector environment answers device tensors: critic_observations() returned "
                                 f"{type(x).__name__}" + (f" on {x.device}" if isinstance(x, torch.Tensor) else ""))
            check_same_device(x.device, self._env_device if dev is None else dev)
            x = x.detach().to(torch.float32)
            x = x.reshape(1, -1) if x.dim() == 1 else x
        else:
            if isinstance(x, torch.Tensor) and x.is_cuda:
                raise ValueError(f"the vector environment speaks the host interface but its critic_observations() returned a tensor on {x.device}")
            x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
            x = x.reshape(1, -1) if x.ndim == 1 else x
        if len(x.shape) != 2 or x.shape[0] != self.n_agents or (self.critic_obs_size is not None and x.shape[1] != self.critic_obs_size):
            raise ValueError(f"the environment's critic_observations() has shape {tuple(x.shape)}: expected [{self.n_agents}, "
                             f"{self.critic_obs_size if self.critic_obs_size is not None else 'd_c'}]")
        return x.contiguous() if isinstance(x, torch.Tensor) else x

    def _critic_init(self):
        """init_processes: the answer after reset() gives d_c, enters critic_obs_stats and is acted on RAW (as the observations)."""
        if not self.critic_observations:
            return
        if not hasattr(self.env, "critic_observations"):
            raise ValueError("critic_observations=True needs a vector environment with a critic_observations() method")
        x = self._critic_answer()
        self.critic_obs_size = int(x.shape[1])
        self.critic_obs_stats = None
        if isinstance(x, torch.Tensor):
            x = x.clone()   # (the environment may reuse its tensor at its first step)
        if self.standardize_obs:
            self.critic_obs_stats = WelfordRunningStat(shape=self.critic_obs_size)
            if isinstance(x, torch.Tensor):
                from ..util import device_stats
                device_stats.increment(self.critic_obs_stats, x)
            else:
                self.critic_obs_stats.increment(x, x.shape[0])
        self._critic_initial = x

    def _critic_begin(self, T, dev):
        """Collect start -> CS [T + 1, n_agents, ld_c], time-major like S, CS[0] = the rows the agents act on now; None when off."""
        if not self.critic_observations:
            return None
        if self.value_net is None:
            raise ValueError("critic_observations: the manager needs the critic (value_net) whose arena stages the rows")
        arena = self.value_net.arena
        CS = torch.empty((T + 1, self.n_agents, arena.ld_in), dtype=torch.float32, device=dev)
        if self._critic_next_rows is None:   # first collect: the reset answer, RAW
            arena.stage_obs(self._critic_initial, None, out=CS[0])
        else:
            CS[0].copy_(self._critic_next_rows)
        return CS

    def _critic_out(self, CS):
        """Collect end: time-major -> trajectory-major once (row a * T + t), + the last next-state row, as value_input_rows."""
        if CS is None:
            return
        T, na, ld = CS.shape[0] - 1, CS.shape[1], CS.shape[2]
        rows = torch.empty((na * T + 1, ld), dtype=torch.float32, device=CS.device)
        rows[:na * T].view(na, T, ld).copy_(CS[:T].transpose(0, 1))
        rows[na * T].copy_(CS[T][na - 1])
        self.critic_value_input_rows = rows
        self._critic_next_rows = CS[T]

    # same signature as BatchedAgentManager.init_processes (learner.py:140-150); n_processes is ignored
    def init_processes(self, n_processes, build_env_fn, collect_metrics_fn=None, spawn_delay=None, render=False,
                       render_delay=None, shm_buffer_size=8192):
        self.env = build_env_fn()
        self.collect_metrics_fn = collect_metrics_fn
        if hasattr(self.env.action_space, "seed"):
            self.env.action_space.seed(self.seed)
        first = self.env.reset()
        self._env_device = device_env_of(first)
        if self._env_device is not None:   # a device-resident environment: _collect_device
            return self._init_device_env(first)
        if isinstance(first, torch.Tensor):   # a CPU tensor: the host interface, held to it (a device step() is refused by name)
            self.env = _HostInterfaceGuard(self.env)
        obs = np.asarray(first, dtype=np.float32)
        self.n_agents, d = obs.shape
        self._ep_rews = np.zeros(self.n_agents, np.float64)
        self.obs_stats = None
        if self.standardize_obs:  # the reset observations enter the statistics and are acted on RAW
            self.obs_stats = WelfordRunningStat(shape=d)                      # (batched_agent_manager.py:366-384)
            self.obs_stats.increment(obs, obs.shape[0])
        self._initial_obs = obs
        self._initial_mask_pending = hasattr(self.env, "action_masks")  # read once the policy exists (first collect)
        self._critic_init()
        n_acts, code = describe_action_space(self.env.action_space)
        return int(np.prod(self.env.observation_space.shape)), int(n_acts), int(code)

    def _standardize_scalars(self, critic=False):
        """critic: of critic_obs_stats (its own cache), for the critic's observation rows."""
        if not self.standardize_obs:
            return None
        stats, slot = (self.critic_obs_stats, "_critic_scalars_cache") if critic else (self.obs_stats, "_scalars_cache")
        key = (id(stats), stats.count, id(stats.running_mean), self.per_feature_obs_standardization)
        cached = getattr(self, slot, None)
        if cached is not None and cached[0] == key:   # the statistics have not moved since (they move every 6th step)
            return cached[1]
        if self.per_feature_obs_standardization:  # device vectors -> rlppo_pad_rows_per_feature
            out = (torch.from_numpy(np.asarray(stats.mean, np.float32).reshape(-1).copy()),
                   torch.from_numpy(np.asarray(stats.std, np.float32).reshape(-1).copy()))
        else:
            out = (float(stats.mean[0]), float(stats.std[0]))
        setattr(self, slot, (key, out))
        return out

    def _final_obs_rows(self, info, dones, truncated, scalars):
        """Environment-side truncations of one step (truncated and not done; `obs` is already the auto-reset observation there):
        -> (agent indices, staged rows of info["final_observation"]) or None.  The rows take the standardisation scalars of that
        step's returned observation and never enter the running statistics."""
        sel = np.flatnonzero((np.asarray(truncated) != 0) & (np.asarray(dones) == 0))
        if sel.size == 0:
            return None
        if not (isinstance(info, dict) and "final_observation" in info):
            if not self._warned_no_final_obs:
                self._warned_no_final_obs = True
                warnings.warn("gae_bootstrap_truncated: the environment truncated an episode but its info has no 'final_observation': "
                              "environment-side truncations bootstrap from the post-reset observation (the truncation at the end of "
                              "every collect is not affected)", RuntimeWarning, stacklevel=3)
            return None
        fo = np.asarray(info["final_observation"], dtype=np.float32).reshape(self.n_agents, -1)[sel]
        return sel, self.policy.arena.stage_obs(np.ascontiguousarray(fo), scalars)

    def _bootstrap_out(self, dones_tm, trunc_tm, nxt_flat, last_rows, patched):
        """Host flags [T, na] of a finished collect (flush rule applied) -> bootstrap_steps / bootstrap_index / bootstrap_rows.
        With no terminal agent at the flush and no other truncation the rows are `last_rows` (the observations the agents act on
        next) as they stand: no index upload and no gather."""
        T, na = dones_tm.shape
        hit = (trunc_tm != 0) & (dones_tm == 0)
        self.bootstrap_steps = np.flatnonzero(hit.T)          # trajectory-major: a * T + t
        if not patched and hit[T - 1].all() and not hit[:T - 1].any():
            self.bootstrap_index, self.bootstrap_rows = None, last_rows
            return
        self.bootstrap_index = torch.from_numpy(self.bootstrap_steps).to(nxt_flat.device)
        self.bootstrap_rows = nxt_flat.index_select(0, self.bootstrap_index)

    @torch.no_grad()
    def collect_timesteps(self, n):
        """-> ((states, actions, log_probs, rewards, next_states, dones, truncated), metrics, n_collected, seconds):
        device tensors in trajectory-major order; `self.value_input_rows` holds states ++ last next_state contiguously."""
        if self._env_device is not None:
            return self._collect_device(n)
        if getattr(self.policy, "fused_step", False):
            return self._collect_fused(n)
        return self._collect_chain(n)

    def _collect_fused(self, n):
        """[r3] The discrete policy's step is ONE launch (DiscreteFF.step -> rlppo_discrete_step): it standardises and pads the raw
        observations of step t straight into the rollout storage, runs the policy, stores the action (as the buffer's float
        encoding) and the log-probability into the storage and the action indices into pinned host memory for the environment.
        The storage is TIME-major while collecting (everything a step writes is contiguous: no scatter copies) and is transposed
        into the reference's trajectory-major order once per collect.  Same numbers as _collect_chain, bit for bit."""
        t1 = time.perf_counter()
        arena = self.policy.arena
        dev, ld, na = arena.device, arena.ld_in, self.n_agents
        T = max(1, -(-int(n) // na))
        N_ = na * T
        S = torch.empty((T + 1, na, ld), dtype=torch.float32, device=dev)     # S[t] = policy-input rows of step t; S[T]: the next collect's
        acts_tm = torch.empty((T, na), dtype=torch.float32, device=dev)
        logp_tm = torch.empty((T, na), dtype=torch.float32, device=dev)
        # [r4] the host side of a step is kept as small as the launch: rewards / flags are TIME-major too (row t is one contiguous
        # write; round 3 wrote three stride-T columns per step) and transposed on the device once per collect; the raw observations
        # go through a small ring of page-locked staging rows (asynchronous upload: a pageable source is copied synchronously);
        # the standardisation scalars are recomputed only when the statistics moved; the episode-reward average runs over the
        # ended agents' values as Python floats (same operations in the same order, no numpy scalar per agent).
        rdt = np.empty((3, T, na), np.float32)                                # rewards, dones, truncated of step t: rdt[:, t]
        metrics = []
        if self._pending_obs is None:  # first collect: the reset observations are acted on RAW (batched_agent_manager.py:366-384)
            self._pending_obs = (torch.from_numpy(np.ascontiguousarray(self._initial_obs)).to(dev), None)
        obs_dev, scalars = self._pending_obs
        stage = self._obs_staging(na, arena.d_in)
        mask, M = self._first_mask(), None
        width = None if mask is None else AM.Layout.of(self.policy).width
        final_rows = []   # bootstrap_truncated: (t, agents, staged final observations) of environment-side truncations
        CS = self._critic_begin(T, dev)
        for t in range(T):
            if mask is not None:
                if M is None:
                    M = torch.empty((T, na, mask.shape[1]), dtype=torch.int32, device=dev)
                M[t].copy_(mask)
            a_host, _ = self.policy.step(obs_dev, standardize=scalars, rows_out=S[t], actions_f32=acts_tm[t], logp_out=logp_tm[t],
                                         to_host="actions", action_mask=None if mask is None else AM.Packed(M[t], width))
            step = self.env.step(a_host.numpy().astype(np.float32).reshape(na, -1))
            if len(step) == 4:
                obs, r, d, info = step
                tr = 0.0
            else:
                obs, r, d, tr, info = step
            if mask is not None:
                mask = self._env_mask()             # describes `obs`, the observation of step t + 1
            pin_t, pin_np = stage[t % len(stage)]   # (reused three steps later: every step ends in a stream synchronisation)
            np.copyto(pin_np, obs, casting="unsafe")
            obs_dev = pin_t.to(dev, non_blocking=True)                         # raw observations: one asynchronous upload per step
            row = rdt[:, t]
            row[0], row[1], row[2] = r, d, tr
            if self.collect_metrics_fn is not None:
                metrics.append(self.collect_metrics_fn(info["state"]))
            scalars = self._standardize_scalars()  # fetched BEFORE this step's increment (batched_agent_manager.py:230-235)
            if self.bootstrap_truncated:
                fin = self._final_obs_rows(info, row[1], row[2], scalars)
                if fin is not None:
                    final_rows.append((t,) + fin)
            if CS is not None:   # the critic's observation of step t + 1, with ITS scalars before this step's increment
                cobs_dev = torch.from_numpy(self._critic_answer()).to(dev)
                cscalars = self._standardize_scalars(critic=True)
            if self.standardize_obs:  # same cadence as one worker response per step
                if self.steps_since_obs_stats_update > self.steps_per_obs_stats_increment:
                    self._increment_obs_stats(obs_dev)
                    if CS is not None:
                        self._increment_obs_stats(cobs_dev, critic=True)
                    self.steps_since_obs_stats_update = 0
                else:
                    self.steps_since_obs_stats_update += 1
            if CS is not None:
                self.value_net.arena.stage_obs(cobs_dev, cscalars, out=CS[t + 1])
            self._track_rewards(row[0], (row[1] + row[2]) > 0)
        arena.stage_obs(obs_dev, scalars, out=S[T])          # the rows the agents act on next = next_states of the last step
        self._pending_obs = (obs_dev, scalars)
        self._pending_mask = mask
        self._masks_out(M, na, T)
        self._critic_out(CS)
        if getattr(self.policy, "noise_mode", None) == "host" and hasattr(self.policy, "prefetch_noise"):
            # the NEXT collect's T draws of the reference's CPU noise stream, produced on the helper threads while the value pass,
            # the GAE scan and PPOLearner.learn run (none of them touches torch's CPU generator; if anything does, the chain is
            # dropped at the next draw: engine.HostExponential)
            self.policy.prefetch_noise(na, T)
        flat = torch.empty((N_ + 1, ld), dtype=torch.float32, device=dev)
        nxt_flat = torch.empty((N_, ld), dtype=torch.float32, device=dev)
        flat[:N_].view(na, T, ld).copy_(S[:T].transpose(0, 1))               # time-major -> trajectory-major, once
        nxt_flat.view(na, T, ld).copy_(S[1:].transpose(0, 1))
        flat[N_].copy_(S[T][na - 1])                         # next_states[-1]: what add_new_experience appends (learner.py:347)
        rdt[2, T - 1] = np.where(rdt[1, T - 1] == 0, 1.0, 0.0)   # flush rule (quirk Q4)
        if self.bootstrap_truncated:
            for t, sel, rows in final_rows:
                nxt_flat[torch.from_numpy(sel * T + t).to(dev)] = rows
            self._bootstrap_out(rdt[1], rdt[2], nxt_flat, S[T], bool(final_rows))
        rdt_dev = torch.from_numpy(rdt).to(dev).transpose(1, 2).contiguous()   # [3, na, T]: trajectory-major, transposed on the device
        self.value_input_rows = flat
        self._next_rows = S[T]
        self.cumulative_timesteps += N_
        experience = (flat[:N_], acts_tm.t().reshape(N_, 1), logp_tm.t().reshape(N_), rdt_dev[0].reshape(N_), nxt_flat,
                      rdt_dev[1].reshape(N_), rdt_dev[2].reshape(N_))
        return experience, metrics, N_, time.perf_counter() - t1

    def _obs_staging(self, na, d):
        """Three page-locked [na, d] float32 staging buffers (tensor, numpy view), allocated once."""
        st = getattr(self, "_stage", None)
        if st is None or st[0][0].shape != (na, d):
            pin = torch.cuda.is_available()
            ts = [torch.empty((na, d), dtype=torch.float32, pin_memory=pin) for _ in range(3)]
            st = self._stage = [(t, t.numpy()) for t in ts]
        return st

    def _collect_chain(self, n):
        t1 = time.perf_counter()
        arena = self.policy.arena
        dev, ld, na = arena.device, arena.ld_in, self.n_agents
        T = max(1, -(-int(n) // na))
        N_ = na * T
        flat = torch.empty((N_ + 1, ld), dtype=torch.float32, device=dev)
        nxt_flat = torch.empty((N_, ld), dtype=torch.float32, device=dev)
        s3, n3 = flat[:N_].view(na, T, ld), nxt_flat.view(na, T, ld)
        acts = logp = None
        rews = np.empty((na, T), np.float32)
        dones = np.empty((na, T), np.float32)
        trunc = np.empty((na, T), np.float32)
        metrics = []
        if self._next_rows is None:
            self._next_rows = arena.stage_obs(self._initial_obs)
        rows = self._next_rows
        mask, M = self._first_mask(), None
        width = None if mask is None else AM.Layout.of(self.policy).width
        patched = False   # bootstrap_truncated: a final observation went into the next-state rows
        CS = self._critic_begin(T, dev)
        for t in range(T):
            if mask is not None:
                if M is None:
                    M = torch.empty((T, na, mask.shape[1]), dtype=torch.int32, device=dev)
                M[t].copy_(mask)
            a_dev, lp_dev = self.policy.act_padded(rows, action_mask=None if mask is None else AM.Packed(M[t], width))
            if acts is None:
                k = 1 if a_dev.dim() == 1 else a_dev.shape[1]
                acts = torch.empty((na, T, k), dtype=torch.float32, device=dev)
                logp = torch.empty((na, T), dtype=torch.float32, device=dev)
            s3[:, t].copy_(rows)
            acts[:, t].copy_(a_dev.view(na, -1))
            logp[:, t].copy_(lp_dev)
            step = self.env.step(a_dev.cpu().numpy().astype(np.float32).reshape(na, -1))
            if len(step) == 4:
                obs, r, d, info = step
                tr = np.zeros(na, np.float32)
            else:
                obs, r, d, tr, info = step
            if mask is not None:
                mask = self._env_mask()             # describes `obs`, the observation of step t + 1
            obs = np.asarray(obs, dtype=np.float32)
            obs_dev = torch.from_numpy(np.ascontiguousarray(obs)).to(dev)   # raw observations: one upload per step
            rews[:, t], dones[:, t], trunc[:, t] = r, d, tr
            if self.collect_metrics_fn is not None:
                metrics.append(self.collect_metrics_fn(info["state"]))
            scalars = self._standardize_scalars()  # fetched BEFORE this step's increment (batched_agent_manager.py:230-235)
            if CS is not None:   # the critic's observation of step t + 1, with ITS scalars before this step's increment
                cobs_dev = torch.from_numpy(self._critic_answer()).to(dev)
                cscalars = self._standardize_scalars(critic=True)
            if self.standardize_obs:  # same cadence as one worker response per step
                if self.steps_since_obs_stats_update > self.steps_per_obs_stats_increment:
                    self._increment_obs_stats(obs_dev)
                    if CS is not None:
                        self._increment_obs_stats(cobs_dev, critic=True)
                    self.steps_since_obs_stats_update = 0
                else:
                    self.steps_since_obs_stats_update += 1
            if CS is not None:
                self.value_net.arena.stage_obs(cobs_dev, cscalars, out=CS[t + 1])
            self._track_rewards(rews[:, t], (dones[:, t] + trunc[:, t]) > 0)
            rows = arena.stage_obs(obs_dev, scalars)
            n3[:, t].copy_(rows)
            if self.bootstrap_truncated:
                fin = self._final_obs_rows(info, dones[:, t], trunc[:, t], scalars)
                if fin is not None:
                    nxt_flat[torch.from_numpy(fin[0] * T + t).to(dev)] = fin[1]
                    patched = True
        flat[N_].copy_(rows[na - 1])                      # next_states[-1]: what add_new_experience appends (learner.py:347)
        trunc[:, T - 1] = np.where(dones[:, T - 1] == 0, 1.0, 0.0)   # flush rule (quirk Q4)
        if self.bootstrap_truncated:
            self._bootstrap_out(dones.T, trunc.T, nxt_flat, rows, patched)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to(dev)
        self.value_input_rows = flat
        self._next_rows = rows
        self._pending_mask = mask
        self._masks_out(M, na, T)
        self._critic_out(CS)
        self.cumulative_timesteps += N_
        experience = (flat[:N_], acts.view(N_, -1), logp.view(N_), up(rews), nxt_flat, up(dones), up(trunc))
        return experience, metrics, N_, time.perf_counter() - t1

    # ------------------------------------------------------------------------------------------ device-resident environment
    def _init_device_env(self, first):
        """init_processes for an environment whose reset() answered a GPU tensor.  The reset observations enter the statistics
        through device_stats.increment (one wait, at start-up) and are acted on RAW, as in the host forms."""
        from ..util import device_stats
        obs = first.detach()
        if obs.dim() != 2:
            raise ValueError(f"a device-resident vector environment's reset() returns [n_agents, d], got {tuple(obs.shape)}")
        obs = obs.to(torch.float32).contiguous().clone()   # (the environment may reuse its tensor at its first step)
        self.n_agents, d = obs.shape
        self.obs_stats = None
        if self.standardize_obs:
            self.obs_stats = WelfordRunningStat(shape=d)
            device_stats.increment(self.obs_stats, obs)
        self._initial_obs = obs
        self._initial_mask_pending = hasattr(self.env, "action_masks")
        self._critic_init()
        n_acts, code = describe_action_space(self.env.action_space)
        return int(np.prod(self.env.observation_space.shape)), int(n_acts), int(code)

    def _env_mask_device(self, dev):
        """action_masks() of a device environment -> packed device words (Layout.pack's device branch: nothing is read back, a row
        without a valid action counts as all-valid); None without the method."""
        fn = getattr(self.env, "action_masks", None)
        if fn is None:
            return None
        lay = AM.Layout.of(self.policy)
        m = fn()
        if not (isinstance(m, torch.Tensor) and m.is_cuda):
            raise ValueError("a device-resident vector environment's action_masks() returns a device tensor [n_agents, width]")
        if m.dim() == 1:
            m = m.view(1, -1)
        if m.dim() != 2 or m.shape[1] != lay.width:
            raise ValueError(f"the environment's action_masks() has shape {tuple(m.shape)}: its width must be {lay.width}, the policy's "
                             + ("logit count sum(bins) (one entry per bin of every component)" if lay.heads is not None else "action count"))
        return lay.pack(m, dev)

    def _book_in(self, dev):
        """Collect start: the host's average and statistics (the host objects own them: checkpoints, Learner.load) go to the device
        through a page-locked buffer, without a wait; the standardisation vectors of the statistics as they stand are computed
        into the pair that the pending observations do not read.  -> the book."""
        from ..engine import ptr, stream_ptr
        from .. import _native as N
        if self._book is None or self._book.device != dev:
            self._book = _DeviceBook(dev, self.n_agents)
        b, st = self._book, self.obs_stats if self.standardize_obs else None
        d = 0 if st is None else int(np.prod(np.shape(st.running_mean)))
        f64 = st is not None and np.asarray(st.running_mean).dtype == np.float64
        b.layout(d, f64)
        host = b.pin.numpy()
        host[:8].view(np.float64)[0] = 0.0 if self.average_reward is None else float(self.average_reward)
        host[8:24].view(np.int64)[:] = (0 if self.average_reward is None else 1, 0)
        if st is not None:
            dt, es = (np.float64, 8) if f64 else (np.float32, 4)
            host[24:24 + d * es].view(dt)[:] = np.asarray(st.running_mean, dt).reshape(-1)
            host[24 + d * es:].view(dt)[:] = np.asarray(st.running_variance, dt).reshape(-1)
        b.blob.copy_(b.pin, non_blocking=True)
        if st is not None:
            pending = self._pending_obs[1] if self._pending_obs is not None else None
            b.cur = 1 if pending is not None and pending[0] is b.vec[0][0] else 0
            N.check(N.lib().rlppo_obs_scalars(stream_ptr(), ptr(b.mean), ptr(b.m2), int(f64), int(st.count), d,
                                              int(bool(self.per_feature_obs_standardization)), ptr(b.vec[b.cur][0]), ptr(b.vec[b.cur][1])))
        return b

    def _book_out(self, b, cb=None):
        """Collect end: ONE device-to-host copy brings back the statistics, the average and the ended-episode count (cb: and the
        critic's statistics, in the same copy)."""
        if cb is not None and cb.blob is not None:
            both = torch.cat((b.blob, cb.blob)).cpu().numpy()
            host, chost = both[:b.blob.numel()], both[b.blob.numel():]
        else:
            host, chost = b.blob.cpu().numpy(), None
        st_words = host[8:24].view(np.int64)
        self.average_reward = float(host[:8].view(np.float64)[0]) if st_words[0] else None
        self.episodes_ended += int(st_words[1])
        for book, st, h in ((b, self.obs_stats, host), (cb, self.critic_obs_stats, chost)):
            if not self.standardize_obs or h is None:
                continue
            dt, es = (np.float64, 8) if book.f64 else (np.float32, 4)
            shape, keep = np.shape(st.running_mean), np.asarray(st.running_mean).dtype
            st.running_mean = h[24:24 + book.d * es].view(dt).reshape(shape).astype(keep, copy=True)
            st.running_variance = h[24 + book.d * es:].view(dt).reshape(shape).astype(keep, copy=True)

    def _critic_book_in(self, dev):
        """_book_in for critic_obs_stats: its state to a _DeviceBook of its own (the 24 state bytes unused) and the standardisation
        vectors of the statistics as they stand; None when the critic's rows are not standardised."""
        from ..engine import ptr, stream_ptr
        from .. import _native as N
        st = self.critic_obs_stats if self.standardize_obs else None
        if st is None:
            return None
        if self._cbook is None or self._cbook.device != dev:
            self._cbook = _DeviceBook(dev, 0)
        cb = self._cbook
        d = int(np.prod(np.shape(st.running_mean)))
        f64 = np.asarray(st.running_mean).dtype == np.float64
        cb.layout(d, f64)
        host = cb.pin.numpy()
        host[:24] = 0
        dt, es = (np.float64, 8) if f64 else (np.float32, 4)
        host[24:24 + d * es].view(dt)[:] = np.asarray(st.running_mean, dt).reshape(-1)
        host[24 + d * es:].view(dt)[:] = np.asarray(st.running_variance, dt).reshape(-1)
        cb.blob.copy_(cb.pin, non_blocking=True)
        cb.cur = 0   # (the critic's rows are staged in the step that fetched their pair: nothing pending reads the other one)
        N.check(N.lib().rlppo_obs_scalars(stream_ptr(), ptr(cb.mean), ptr(cb.m2), int(f64), int(st.count), d,
                                          int(bool(self.per_feature_obs_standardization)), ptr(cb.vec[0][0]), ptr(cb.vec[0][1])))
        return cb

    def _collect_device(self, n):
        """The collect of a DEVICE-RESIDENT environment (reset() / step() answer GPU tensors on torch's current stream): the numbers of
        _collect_fused / _collect_chain, bit for bit, with nothing between two steps on the host -- per step the policy's launch (the
        one-launch step with device standardisation vectors; other heads: stage_obs + act_padded), a copy of the action row for the
        environment, the environment's own work and ONE rlppo_rollout_record (rewards / flags into the time-major planes, episode
        sums and the 0.9 / 0.1 average in agent order); on the steps where the statistics move, rlppo_welford_increment on the
        device state and rlppo_obs_scalars.  The host enqueues and never waits; it reads back once, at the end (_book_out)."""
        from ..engine import _resolve_device, ptr, stream_ptr
        from .. import _native as N
        t1 = time.perf_counter()
        arena = self.policy.arena
        dev, ld, na = _resolve_device(arena.device), arena.ld_in, self.n_agents
        check_same_device(self._env_device, dev)
        L = N.lib()
        fused = bool(getattr(self.policy, "fused_step", False))
        T = max(1, -(-int(n) // na))
        N_ = na * T
        S = torch.empty((T + 1, na, ld), dtype=torch.float32, device=dev)     # time-major, as in _collect_fused
        logp_tm = torch.empty((T, na), dtype=torch.float32, device=dev)
        acts_tm = torch.empty((T, na, 1), dtype=torch.float32, device=dev) if fused else None
        rdt = torch.empty((3, T, na), dtype=torch.float32, device=dev)
        metrics = []
        b = self._book_in(dev)
        CS = self._critic_begin(T, dev)
        cb = self._critic_book_in(dev) if CS is not None else None
        if self._pending_obs is None:   # first collect: the reset observations are acted on RAW
            self._pending_obs = (self._initial_obs, None)
        obs_dev, scalars = self._pending_obs
        if not fused:
            arena.stage_obs(obs_dev, scalars, out=S[0])
        if self._initial_mask_pending:
            self._initial_mask_pending = False
            self._pending_mask = self._env_mask_device(dev)
        mask, M = self._pending_mask, None
        width = None if mask is None else AM.Layout.of(self.policy).width
        F = P = None   # bootstrap_truncated: staged final observations [T, na, ld] and the patch plane [T, na], allocated on first use
        for t in range(T):
            am = None
            if mask is not None:
                if M is None:
                    M = torch.empty((T, na, mask.shape[1]), dtype=torch.int32, device=dev)
                M[t].copy_(mask)
                am = AM.Packed(M[t], width)
            if fused:
                self.policy.step(obs_dev, standardize=scalars, rows_out=S[t], actions_f32=acts_tm[t].view(na), logp_out=logp_tm[t],
                                 to_host=False, action_mask=am)
                a_env = acts_tm[t].clone()
            else:
                a_dev, lp_dev = self.policy.act_padded(S[t], action_mask=am)
                a_dev = a_dev.view(na, -1)
                if acts_tm is None:
                    acts_tm = torch.empty((T, na, a_dev.shape[1]), dtype=torch.float32, device=dev)
                acts_tm[t].copy_(a_dev)
                logp_tm[t].copy_(lp_dev)
                a_env = a_dev.to(torch.float32)   # (act_padded's own output or a conversion of it: never the storage)
            step = self.env.step(a_env)
            if len(step) == 4:
                obs, r, d, info = step
                tr = None
            else:
                obs, r, d, tr, info = step
            if not (isinstance(obs, torch.Tensor) and obs.is_cuda):
                raise ValueError("a device-resident vector environment answers device tensors: step() returned observations as "
                                 f"{type(obs).__name__}" + (f" on {obs.device}" if isinstance(obs, torch.Tensor) else ""))
            check_same_device(obs.device, dev)
            obs_dev = obs.detach().to(torch.float32).reshape(na, -1).contiguous()
            if mask is not None:
                mask = self._env_mask_device(dev)   # describes `obs`, the observation of step t + 1
            if self.collect_metrics_fn is not None:
                metrics.append(self.collect_metrics_fn(info["state"]))
            scalars = b.vec[b.cur] if self.standardize_obs else None   # the pair BEFORE this step's increment
            patch_t = None
            if self.bootstrap_truncated:
                if isinstance(info, dict) and "final_observation" in info:
                    if F is None:
                        F = torch.empty((T, na, ld), dtype=torch.float32, device=dev)
                        P = torch.zeros((T, na), dtype=torch.float32, device=dev)
                    arena.stage_obs(info["final_observation"].reshape(na, -1), scalars, out=F[t])
                    patch_t = P[t]
                elif not self._warned_no_final_obs:   # (decided by the key alone: nothing on the device is read)
                    self._warned_no_final_obs = True
                    warnings.warn("gae_bootstrap_truncated: the environment's info has no 'final_observation': environment-side "
                                  "truncations bootstrap from the post-reset observation (the truncation at the end of every collect "
                                  "is not affected)", RuntimeWarning, stacklevel=3)
            if CS is not None:   # the critic's observation of step t + 1, staged with ITS pair before this step's increment
                cobs_dev = self._critic_answer(dev)
                self.value_net.arena.stage_obs(cobs_dev, None if cb is None else cb.vec[cb.cur], out=CS[t + 1])
            if self.standardize_obs:   # the host forms' cadence; the sample count is the host's
                if self.steps_since_obs_stats_update > self.steps_per_obs_stats_increment:
                    st = self.obs_stats
                    N.check(L.rlppo_welford_increment(stream_ptr(), ptr(obs_dev), obs_dev.stride(0), na, b.d, ptr(b.mean), ptr(b.m2),
                                                      int(st.count), int(b.f64)))
                    st.count += na
                    b.cur = 1 - b.cur
                    N.check(L.rlppo_obs_scalars(stream_ptr(), ptr(b.mean), ptr(b.m2), int(b.f64), int(st.count), b.d,
                                                int(bool(self.per_feature_obs_standardization)), ptr(b.vec[b.cur][0]), ptr(b.vec[b.cur][1])))
                    if cb is not None:   # critic_obs_stats moves with obs_stats, on its own device state
                        cst = self.critic_obs_stats
                        N.check(L.rlppo_welford_increment(stream_ptr(), ptr(cobs_dev), cobs_dev.stride(0), na, cb.d, ptr(cb.mean), ptr(cb.m2),
                                                          int(cst.count), int(cb.f64)))
                        cst.count += na
                        cb.cur = 1 - cb.cur
                        N.check(L.rlppo_obs_scalars(stream_ptr(), ptr(cb.mean), ptr(cb.m2), int(cb.f64), int(cst.count), cb.d,
                                                    int(bool(self.per_feature_obs_standardization)), ptr(cb.vec[cb.cur][0]), ptr(cb.vec[cb.cur][1])))
                    self.steps_since_obs_stats_update = 0
                else:
                    self.steps_since_obs_stats_update += 1
            r, r_dt = _dt_code(r, "rewards", dev, na)
            if r_dt == 2:
                r, r_dt = r.to(torch.float32), 0
            d, d_dt = _dt_code(d, "dones", dev, na)
            tr, tr_dt = (None, 0) if tr is None else _dt_code(tr, "truncated", dev, na)
            N.check(L.rlppo_rollout_record(stream_ptr(), ptr(r), r_dt, ptr(d), d_dt, ptr(tr), tr_dt, na, t, T, ptr(rdt), ptr(b.ep_sums),
                                           ptr(b.state), ptr(patch_t)))
            if not fused or t == T - 1:
                arena.stage_obs(obs_dev, scalars, out=S[t + 1])   # the rows the agents act on next
        self._pending_obs = (obs_dev, scalars)
        self._pending_mask = mask
        self._masks_out(M, na, T)
        self._critic_out(CS)
        if getattr(self.policy, "noise_mode", None) == "host" and hasattr(self.policy, "prefetch_noise"):
            self.policy.prefetch_noise(na, T)   # as _collect_fused: the next collect's draws, produced while the update runs
        k = acts_tm.shape[2]
        flat = torch.empty((N_ + 1, ld), dtype=torch.float32, device=dev)
        nxt_flat = torch.empty((N_, ld), dtype=torch.float32, device=dev)
        actions = torch.empty((N_, k), dtype=torch.float32, device=dev)
        small = torch.empty((4, N_), dtype=torch.float32, device=dev)   # log_probs, rewards, dones, truncated
        N.check(L.rlppo_rollout_to_trajectory_major(stream_ptr(), ptr(S), ptr(acts_tm), ptr(logp_tm), ptr(rdt), na, T, ld, k, ptr(P), ptr(F),
                                                    ptr(flat), ptr(nxt_flat), ptr(actions), ptr(small[0]), ptr(small[1]), ptr(small[2]),
                                                    ptr(small[3])))
        if self.bootstrap_truncated:   # the host does not know which steps are truncated: all N next-state rows, the scan selects
            self.bootstrap_dense, self.bootstrap_steps, self.bootstrap_index, self.bootstrap_rows = True, None, None, nxt_flat
        self.value_input_rows = flat
        self._next_rows = S[T]
        self.cumulative_timesteps += N_
        self.last_enqueue_seconds = time.perf_counter() - t1   # host time of the whole collect before its one wait
        self._book_out(b, cb)
        experience = (flat[:N_], actions, small[0], small[1], nxt_flat, small[2], small[3])
        return experience, metrics, N_, time.perf_counter() - t1

    def _first_mask(self):
        """The mask of the observation a collect starts on: the one left by the previous collect, or -- first collect -- the
        environment's answer after its reset()."""
        if self._initial_mask_pending:
            self._initial_mask_pending = False
            self._pending_mask = self._env_mask()
        return self._pending_mask

    def _increment_obs_stats(self, obs_dev, critic=False):
        """WelfordRunningStat.increment(obs, n) on the device (bit-exact with the host class's sample-by-sample update in the
        state's dtype -- float32, or float64 after a checkpoint load -- which costs ~10 ms of Python per 4096 samples); the host
        object stays the owner of the state (checkpoints)."""
        from ..util import device_stats
        device_stats.increment(self.critic_obs_stats if critic else self.obs_stats, obs_dev)

    def _track_rewards(self, r, ended):
        """Episode-reward average as batched_agent_manager.py:377-399 keeps it, one agent = one stream: the ended agents' episode
        sums enter the 0.9 / 0.1 average in agent order (Python floats, the reference's operations in the reference's order)."""
        self._ep_rews += r
        idx = np.flatnonzero(ended)
        if idx.size == 0:
            return
        avg = self.average_reward
        for x in self._ep_rews[idx].tolist():
            avg = x if avg is None else avg * 0.9 + x * 0.1
        self.average_reward = avg
        self._ep_rews[idx] = 0.0

    def cleanup(self):
        if self.env is not None and hasattr(self.env, "close"):
            self.env.close()
        self.env = None
