"""Rollout collection for ONE vectorised environment that steps all of its agents in lockstep, with the rollout kept on
the GPU (device-resident rollout storage, vector-env fast path).

The reference collects through one OS process per environment, a UDP datagram per step and Python lists per agent
(batched_agent_manager.py:126-299, batched_trajectory.py:58-105); at 4096 agents that is 4096 datagrams per step and,
per iteration, seven `np.asarray` flattens plus a 224 MB upload of the states.  Here the policy's padded input rows of
step t are written on the device, TIME-major while collecting (everything a step writes is contiguous), and moved into
their final, trajectory-major position (row a*T + t of agent a) by one launch per collect, so
`Learner.add_new_experience` runs the value pass, the GAE scan and the buffer submit on them without a copy through the host.

What comes out is exactly what the reference's assembler would produce for the same interaction sequence when every agent
is its own trajectory stream (tests/test_gpu_vector_rollout.py compares with a numpy restatement of these rules):
  * trajectories are concatenated agent by agent, steps in order (batched_trajectory.py:58-105);
  * the last collected step of every agent is force-marked truncated unless it is terminal (quirk Q4, the flush at
    batched_agent_manager.py:154-172), and the episode continues in the next collect;
  * observations are standardised with the SCALAR statistics of feature 0 and clipped to +-5 (quirk Q5, :303-315), the
    running statistics are advanced every `steps_per_obs_stats_increment` steps with the raw observations (:233-235);
  * `next_states[i]` is the observation the environment returned for step i (after its auto-reset at episode ends).

ONE step loop (`collect_timesteps`) serves every environment and every policy head.  It talks to two small sides:
  * the ENVIRONMENT's side, `_HostEnv` (numpy) or `_DeviceEnv` (an environment on the GPU), chosen by what `reset()` answered.
    It turns `step()`'s answer into raw float32 device observations, records rewards and flags, owns the standardisation pair and
    the statistics increment, reads `action_masks()` / `critic_observations()`, stages final observations and closes the collect;
  * the HEAD's side, `_act`: `policy.step` (one launch: standardise, pad into S[t], act) for a policy with `fused_step`, else
    `arena.stage_obs` + `act_padded`.
Storage is time-major for all of them -- S[T + 1, na, ld], acts[T, na, k], logp[T, na], CS[T + 1, na, ld_c], M[T, na, W] -- and what
carries over between collects is one thing: the raw pending observation with its pair, S[T] (`_next_rows`), CS[T] and the pending
mask; `policy.fused_step` may change between collects.  All forms give the same numbers, bit for bit
(tests/test_gpu_vector_collect_forms.py).

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

Device interface (an environment that itself lives on the GPU; chosen when `reset()` answers a torch.Tensor on a GPU: `_DeviceEnv`):
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

from .. import _native as N
from ..engine import _resolve_device, ptr, stream_ptr
from ..util import action_mask as AM
from ..util import device_stats
from ..util.running_stats import WelfordRunningStat
from .batched_agent import describe_action_space


def device_env_of(first_obs):
    """Which interface an environment speaks, judged by what its reset() answered: the torch.device of a tensor on a GPU (the device
    interface, _DeviceEnv), or None (numpy arrays, lists, CPU tensors: the host interface, _HostEnv)."""
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


def _device_answer(x, what):
    """A device environment's answer must be a tensor on a GPU; `what` names it in the error."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise ValueError(f"a device-resident vector environment answers device tensors: {what} as "
                         f"{type(x).__name__}" + (f" on {x.device}" if isinstance(x, torch.Tensor) else ""))


def _dt_code(x, what, device, n):
    """Device array of one step (rewards / flags) -> (tensor the record kernel reads, dtype code)."""
    _device_answer(x, f"step() returned {what}")
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
    """One running statistic as _DeviceEnv keeps it on the device between environment steps, one allocation read back in ONE copy
    per collect:
    blob = [ state: int64[3] = bits of the double episode-reward average, has-value word, ended-episode counter (the critic's book
             leaves them unused) |
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

    def load(self, stats, per_feature, average=None, pending=None):
        """Collect start: the host's average and statistics (the host objects own them: checkpoints, Learner.load) go to the device
        through a page-locked buffer, without a wait; the standardisation vectors of the statistics as they stand are computed
        into the pair that the pending observations (their pair: `pending`) do not read.  stats None: not standardised."""
        d = 0 if stats is None else int(np.prod(np.shape(stats.running_mean)))
        f64 = stats is not None and np.asarray(stats.running_mean).dtype == np.float64
        self.layout(d, f64)
        host = self.pin.numpy()
        host[:8].view(np.float64)[0] = 0.0 if average is None else float(average)
        host[8:24].view(np.int64)[:] = (0 if average is None else 1, 0)
        if stats is not None:
            dt, es = (np.float64, 8) if f64 else (np.float32, 4)
            host[24:24 + d * es].view(dt)[:] = np.asarray(stats.running_mean, dt).reshape(-1)
            host[24 + d * es:].view(dt)[:] = np.asarray(stats.running_variance, dt).reshape(-1)
        self.blob.copy_(self.pin, non_blocking=True)
        if stats is not None:
            self.cur = 1 if pending is not None and pending[0] is self.vec[0][0] else 0
            self._scalars(stats.count, per_feature)

    def _scalars(self, count, per_feature):
        N.check(N.lib().rlppo_obs_scalars(stream_ptr(), ptr(self.mean), ptr(self.m2), int(self.f64), int(count), self.d,
                                          int(bool(per_feature)), ptr(self.vec[self.cur][0]), ptr(self.vec[self.cur][1])))

    def advance(self, x, stats, per_feature):
        """The statistics take the rows x [n, d] on the device (the sample count is the host's) and the OTHER pair takes their vectors."""
        N.check(N.lib().rlppo_welford_increment(stream_ptr(), ptr(x), x.stride(0), x.shape[0], self.d, ptr(self.mean), ptr(self.m2),
                                                int(stats.count), int(self.f64)))
        stats.count += x.shape[0]
        self.cur = 1 - self.cur
        self._scalars(stats.count, per_feature)

    def store(self, stats, host):
        """Collect end: the bytes read back from `blob` -> the host statistics, in their own dtype."""
        dt, es = (np.float64, 8) if self.f64 else (np.float32, 4)
        shape, keep = np.shape(stats.running_mean), np.asarray(stats.running_mean).dtype
        stats.running_mean = host[24:24 + self.d * es].view(dt).reshape(shape).astype(keep, copy=True)
        stats.running_variance = host[24 + self.d * es:].view(dt).reshape(shape).astype(keep, copy=True)


class _HostEnv(object):
    """The environment's side of the collect loop, HOST interface (numpy).  Per step the host work is kept as small as the launch:
    the raw observations go through a small ring of page-locked staging rows (asynchronous upload: a pageable source is copied
    synchronously); rewards / flags are numpy, TIME-major (row t is one contiguous write) and uploaded once per collect; the
    standardisation scalars are recomputed only when the statistics moved; the episode-reward average runs over the ended agents'
    values as Python floats.  No rlppo_rollout_record launch."""
    to_host = "actions"   # what DiscreteFF.step hands back: the action indices in pinned host memory

    def __init__(self, mgr):
        self.m, self.ring, self.ep_rews = mgr, None, None

    def first_observation(self, first):
        obs = np.asarray(first, dtype=np.float32)
        self.ep_rews = np.zeros(obs.shape[0], np.float64)
        return obs

    def enter_stats(self, stats, x):
        stats.increment(x, x.shape[0])

    def begin(self, T, dev):
        na, d = self.m.n_agents, self.m.policy.arena.d_in
        if self.ring is None or self.ring[0][0].shape != (na, d):   # three page-locked [na, d] buffers (tensor, numpy view)
            ts = [torch.empty((na, d), dtype=torch.float32, pin_memory=torch.cuda.is_available()) for _ in range(3)]
            self.ring = [(t, t.numpy()) for t in ts]
        self.dev, self.rdt = dev, np.empty((3, T, na), np.float32)   # rewards, dones, truncated of step t: rdt[:, t]
        self.final_rows = []   # bootstrap_truncated: (t, agents, staged final observations) of environment-side truncations

    def upload(self, x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)

    def action(self, a):
        return a.cpu().numpy().astype(np.float32).reshape(self.m.n_agents, -1)

    def observations(self, t, obs):
        pin_t, pin_np = self.ring[t % len(self.ring)]   # (reused three steps later: every step ends in a stream synchronisation)
        np.copyto(pin_np, obs, casting="unsafe")
        return pin_t.to(self.dev, non_blocking=True)    # raw observations: one asynchronous upload per step

    def mask(self, m):
        return np.asarray(m)

    def critic(self, x):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            raise ValueError(f"the vector environment speaks the host interface but its critic_observations() returned a tensor on {x.device}")
        return np.ascontiguousarray(np.asarray(x, dtype=np.float32))

    def pair(self, critic=False):
        return self.m._standardize_scalars(critic=True) if critic else self.m._standardize_scalars()

    def increment(self, obs_dev, cobs_dev):
        self.m._increment_obs_stats(obs_dev)
        if cobs_dev is not None:
            self.m._increment_obs_stats(cobs_dev, critic=True)

    def record(self, t, r, d, tr, info, pair):
        row = self.rdt[:, t]
        row[0], row[1], row[2] = r, d, (0.0 if tr is None else tr)
        if self.m.bootstrap_truncated:
            fin = self._final_obs_rows(info, row[1], row[2], pair)
            if fin is not None:
                self.final_rows.append((t,) + fin)
        self._track_rewards(row[0], (row[1] + row[2]) > 0)

    def _final_obs_rows(self, info, dones, truncated, scalars):
        """Environment-side truncations of one step (truncated and not done; `obs` is already the auto-reset observation there):
        -> (agent indices, staged rows of info["final_observation"]) or None.  The rows take the standardisation scalars of that
        step's returned observation and never enter the running statistics."""
        sel = np.flatnonzero((truncated != 0) & (dones == 0))
        if sel.size == 0:
            return None
        if not (isinstance(info, dict) and "final_observation" in info):
            if not self.m._warned_no_final_obs:
                self.m._warned_no_final_obs = True
                warnings.warn("gae_bootstrap_truncated: the environment truncated an episode but its info has no 'final_observation': "
                              "environment-side truncations bootstrap from the post-reset observation (the truncation at the end of "
                              "every collect is not affected)", RuntimeWarning, stacklevel=4)
            return None
        fo = np.asarray(info["final_observation"], dtype=np.float32).reshape(self.m.n_agents, -1)[sel]
        return sel, self.m.policy.arena.stage_obs(np.ascontiguousarray(fo), scalars)

    def _track_rewards(self, r, ended):
        """Episode-reward average as batched_agent_manager.py:377-399 keeps it, one agent = one stream: the ended agents' episode
        sums enter the 0.9 / 0.1 average in agent order (Python floats, the reference's operations in the reference's order)."""
        self.ep_rews += r
        idx = np.flatnonzero(ended)
        if idx.size == 0:
            return
        avg = self.m.average_reward
        for x in self.ep_rews[idx].tolist():
            avg = x if avg is None else avg * 0.9 + x * 0.1
        self.m.average_reward = avg
        self.ep_rews[idx] = 0.0

    def planes(self):
        """-> (rdt on the device, patch plane, final rows): the flush rule (quirk Q4) applied here, ONE upload, no patch planes."""
        T = self.rdt.shape[1]
        self.rdt[2, T - 1] = np.where(self.rdt[1, T - 1] == 0, 1.0, 0.0)
        return torch.from_numpy(self.rdt).to(self.dev), None, None

    def finish(self, nxt_flat, last_rows, t1):
        """The sparse final-observation rows into the transposed next states, then bootstrap_steps / bootstrap_index /
        bootstrap_rows.  With no terminal agent at the flush and no other truncation the rows are `last_rows` (the observations
        the agents act on next) as they stand: no index upload and no gather."""
        m = self.m
        if not m.bootstrap_truncated:
            return
        T = self.rdt.shape[1]
        for t, sel, rows in self.final_rows:
            nxt_flat[torch.from_numpy(sel * T + t).to(self.dev)] = rows
        hit = (self.rdt[2] != 0) & (self.rdt[1] == 0)
        m.bootstrap_steps = np.flatnonzero(hit.T)          # trajectory-major: a * T + t
        if not self.final_rows and hit[T - 1].all() and not hit[:T - 1].any():
            m.bootstrap_index, m.bootstrap_rows = None, last_rows
            return
        m.bootstrap_index = torch.from_numpy(m.bootstrap_steps).to(self.dev)
        m.bootstrap_rows = nxt_flat.index_select(0, m.bootstrap_index)


class _DeviceEnv(object):
    """The environment's side of the collect loop, DEVICE interface (reset() / step() answer GPU tensors on torch's current stream):
    nothing between two steps on the host -- per step ONE rlppo_rollout_record (rewards / flags into the time-major planes, episode
    sums and the 0.9 / 0.1 average in agent order); on the steps where the statistics move, the Welford increment on the device
    state and rlppo_obs_scalars (_DeviceBook.advance).  The host enqueues and never waits; it reads back once, in finish()."""
    to_host = False

    def __init__(self, mgr):
        self.m, self.book, self.cbook = mgr, None, None

    def first_observation(self, first):
        obs = first.detach()
        if obs.dim() != 2:
            raise ValueError(f"a device-resident vector environment's reset() returns [n_agents, d], got {tuple(obs.shape)}")
        return obs.to(torch.float32).contiguous().clone()   # (the environment may reuse its tensor at its first step)

    def enter_stats(self, stats, x):
        device_stats.increment(stats, x)   # (one wait, at start-up)

    def begin(self, T, dev):
        m, na = self.m, self.m.n_agents
        check_same_device(m._env_device, dev)
        if self.book is None or self.book.device != dev:
            self.book, self.cbook = _DeviceBook(dev, na), _DeviceBook(dev, 0)
        self.dev = dev
        self.rdt = torch.empty((3, T, na), dtype=torch.float32, device=dev)
        self.F = self.P = None   # bootstrap_truncated: staged final observations [T, na, ld] and the patch plane [T, na], on first use
        pending = m._pending_obs[1] if m._pending_obs is not None else None
        self.book.load(m.obs_stats if m.standardize_obs else None, m.per_feature_obs_standardization, m.average_reward, pending)
        # (the critic's rows are staged in the step that fetched their pair: nothing pending reads the other one)
        self.critic_standardized = bool(m.critic_observations and m.standardize_obs and m.critic_obs_stats is not None)
        if self.critic_standardized:
            self.cbook.load(m.critic_obs_stats, m.per_feature_obs_standardization)

    def upload(self, x):
        return x

    def action(self, a):
        return a.view(self.m.n_agents, -1).to(torch.float32)   # (the head's own output or a conversion of it: never the storage)

    def observations(self, t, obs):
        _device_answer(obs, "step() returned observations")
        check_same_device(obs.device, self.dev)
        return obs.detach().to(torch.float32).reshape(self.m.n_agents, -1).contiguous()

    def mask(self, m):
        if not (isinstance(m, torch.Tensor) and m.is_cuda):
            raise ValueError("a device-resident vector environment's action_masks() returns a device tensor [n_agents, width]")
        return m

    def critic(self, x):
        _device_answer(x, "critic_observations() returned")
        check_same_device(x.device, self.m._env_device)
        return x.detach().to(torch.float32)

    def pair(self, critic=False):
        if critic:
            return self.cbook.vec[self.cbook.cur] if self.critic_standardized else None
        return self.book.vec[self.book.cur] if self.m.standardize_obs else None

    def increment(self, obs_dev, cobs_dev):
        m = self.m
        self.book.advance(obs_dev, m.obs_stats, m.per_feature_obs_standardization)
        if cobs_dev is not None and self.critic_standardized:   # critic_obs_stats moves with obs_stats, on its own device state
            self.cbook.advance(cobs_dev, m.critic_obs_stats, m.per_feature_obs_standardization)

    def record(self, t, r, d, tr, info, pair):
        m, na, b = self.m, self.m.n_agents, self.book
        T = self.rdt.shape[1]
        patch_t = None
        if m.bootstrap_truncated:
            if isinstance(info, dict) and "final_observation" in info:
                if self.F is None:
                    self.F = torch.empty((T, na, m.policy.arena.ld_in), dtype=torch.float32, device=self.dev)
                    self.P = torch.zeros((T, na), dtype=torch.float32, device=self.dev)
                m.policy.arena.stage_obs(info["final_observation"].reshape(na, -1), pair, out=self.F[t])
                patch_t = self.P[t]
            elif not m._warned_no_final_obs:   # (decided by the key alone: nothing on the device is read)
                m._warned_no_final_obs = True
                warnings.warn("gae_bootstrap_truncated: the environment's info has no 'final_observation': environment-side "
                              "truncations bootstrap from the post-reset observation (the truncation at the end of every collect "
                              "is not affected)", RuntimeWarning, stacklevel=3)
        r, r_dt = _dt_code(r, "rewards", self.dev, na)
        if r_dt == 2:
            r, r_dt = r.to(torch.float32), 0
        d, d_dt = _dt_code(d, "dones", self.dev, na)
        tr, tr_dt = (None, 0) if tr is None else _dt_code(tr, "truncated", self.dev, na)
        N.check(N.lib().rlppo_rollout_record(stream_ptr(), ptr(r), r_dt, ptr(d), d_dt, ptr(tr), tr_dt, na, t, T, ptr(self.rdt),
                                             ptr(b.ep_sums), ptr(b.state), ptr(patch_t)))

    def planes(self):
        return self.rdt, self.P, self.F

    def finish(self, nxt_flat, last_rows, t1):
        """ONE device-to-host copy brings back the statistics, the average and the ended-episode count (and the critic's statistics,
        in the same copy).  The host does not know which steps are truncated: bootstrap_rows are all N next-state rows."""
        m, b, cb = self.m, self.book, self.cbook
        if m.bootstrap_truncated:
            m.bootstrap_dense, m.bootstrap_steps, m.bootstrap_index, m.bootstrap_rows = True, None, None, nxt_flat
        m.last_enqueue_seconds = time.perf_counter() - t1   # host time of the whole collect before its one wait
        if self.critic_standardized:
            both = torch.cat((b.blob, cb.blob)).cpu().numpy()
            host, chost = both[:b.blob.numel()], both[b.blob.numel():]
            cb.store(m.critic_obs_stats, chost)
        else:
            host = b.blob.cpu().numpy()
        st_words = host[8:24].view(np.int64)
        m.average_reward = float(host[:8].view(np.float64)[0]) if st_words[0] else None
        m.episodes_ended += int(st_words[1])
        if m.standardize_obs:
            b.store(m.obs_stats, host)
        self.rdt = self.F = self.P = None


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
        # what carries over between collects, the same for every form:
        self._pending_obs = None      # (raw device observations, their standardisation pair) the agents act on next
        self._next_rows = None        # S[T]: the padded device rows of that observation
        self._pending_mask = None     # packed device words [n_agents, W] of that observation
        self._critic_next_rows = None          # CS[T]: [n_agents, ld_c] staged critic rows of that observation
        self.action_mask_rows = None  # util.action_mask.Packed [N, W] of the last collect (trajectory-major), or None: env without masks
        # Learner(gae_bootstrap_truncated=True): every collect leaves what the bootstrap form of the GAE scan needs; off, a collect
        # does exactly what it did without the option
        self.bootstrap_truncated = False
        self.bootstrap_steps = None   # int64 host indices (trajectory-major) of the steps with truncated and not done
        self.bootstrap_index = None   # the same on the device; None when they are exactly the last step of every agent (the flush)
        self.bootstrap_rows = None    # [m, ld] device rows: the next states of those steps, in the order of bootstrap_steps
        self.bootstrap_dense = False  # True (device environment): bootstrap_rows are ALL N next-state rows, the scan selects by the flags
        self._warned_no_final_obs = False
        self._env_device = None       # torch.device of a device-resident environment (its reset() answered a GPU tensor), else None
        self._env_side = None         # _HostEnv / _DeviceEnv: the environment's side of the collect loop
        self._initial_mask_pending = False
        self.last_enqueue_seconds = None   # device environment: host seconds the last collect spent enqueuing, before its one read
        self.episodes_ended = 0       # device environment: episodes ended so far (read back with the average at the end of a collect)
        # Learner(critic_observations=True): the critic's own observation rows (module docstring); off, a collect does what it did
        self.critic_observations = False
        self.value_net = None                  # the critic (its arena stages the rows); set by Learner once it exists
        self.critic_obs_size = None            # d_c, from the environment's first answer
        self.critic_obs_stats = None           # WelfordRunningStat(d_c), moved when obs_stats moves
        self.critic_value_input_rows = None    # [N + 1, ld_c] device rows of the last collect, mirroring value_input_rows
        self._critic_initial = None            # the answer after reset(): acted on RAW by the first collect

    def _side(self):
        """The environment's side for the interface the environment speaks (`_env_device`), made on first use and kept."""
        kind = _HostEnv if self._env_device is None else _DeviceEnv
        if type(self._env_side) is not kind:
            self._env_side = kind(self)
        return self._env_side

    def _env_mask(self):
        """The environment's action_masks() for the observation the agents act on next, packed on the device (a device environment:
        Layout.pack's device branch, nothing is read back, a row without a valid action counts as all-valid); None without it."""
        fn = getattr(self.env, "action_masks", None)
        if fn is None:
            return None
        lay = AM.Layout.of(self.policy)
        m = self._side().mask(fn())
        if m.ndim == 1:   # a one-agent environment may answer [n_actions]
            m = m.reshape(1, -1)
        if m.ndim != 2 or m.shape[1] != lay.width:
            raise ValueError(f"the environment's action_masks() has shape {tuple(m.shape)}: its width must be {lay.width}, the policy's "
                             + ("logit count sum(bins) (one entry per bin of every component)" if lay.heads is not None else "action count"))
        return lay.pack(m, self.policy.arena.device)

    @property
    def action_masks(self):
        """bool [N, n_actions] of the last collect, trajectory-major; None when the environment has no action_masks()."""
        return None if self.action_mask_rows is None else self.action_mask_rows.unpack()

    def _critic_answer(self):
        """The environment's critic_observations() for the observation the agents act on next: host interface -> float32 numpy
        [n_agents, d_c]; device interface -> float32 device tensor."""
        x = self._side().critic(self.env.critic_observations())
        x = x.reshape(1, -1) if x.ndim == 1 else x
        if x.ndim != 2 or x.shape[0] != self.n_agents or (self.critic_obs_size is not None and x.shape[1] != self.critic_obs_size):
            raise ValueError(f"the environment's critic_observations() has shape {tuple(x.shape)}: expected [{self.n_agents}, "
                             f"{self.critic_obs_size if self.critic_obs_size is not None else 'd_c'}]")
        return x.contiguous() if isinstance(x, torch.Tensor) else x

    # same signature as BatchedAgentManager.init_processes (learner.py:140-150); n_processes is ignored
    def init_processes(self, n_processes, build_env_fn, collect_metrics_fn=None, spawn_delay=None, render=False,
                       render_delay=None, shm_buffer_size=8192):
        self.env = build_env_fn()
        self.collect_metrics_fn = collect_metrics_fn
        if hasattr(self.env.action_space, "seed"):
            self.env.action_space.seed(self.seed)
        first = self.env.reset()
        self._env_device = device_env_of(first)
        if self._env_device is None and isinstance(first, torch.Tensor):
            self.env = _HostInterfaceGuard(self.env)   # a CPU tensor: the host interface, held to it (a device step() is refused by name)
        self._env_side = None
        side = self._side()
        obs = side.first_observation(first)
        self.n_agents, d = obs.shape
        self.obs_stats = None
        if self.standardize_obs:  # the reset observations enter the statistics and are acted on RAW (batched_agent_manager.py:366-384)
            self.obs_stats = WelfordRunningStat(shape=d)
            side.enter_stats(self.obs_stats, obs)
        self._initial_obs = obs
        self._initial_mask_pending = hasattr(self.env, "action_masks")  # read once the policy exists (first collect)
        if self.critic_observations:   # the answer after reset() gives d_c, enters critic_obs_stats and is acted on RAW too
            if not hasattr(self.env, "critic_observations"):
                raise ValueError("critic_observations=True needs a vector environment with a critic_observations() method")
            x = self._critic_answer()
            self.critic_obs_size = int(x.shape[1])
            self.critic_obs_stats = None
            if isinstance(x, torch.Tensor):
                x = x.clone()   # (the environment may reuse its tensor at its first step)
            if self.standardize_obs:
                self.critic_obs_stats = WelfordRunningStat(shape=self.critic_obs_size)
                side.enter_stats(self.critic_obs_stats, x)
            self._critic_initial = x
        n_acts, code = describe_action_space(self.env.action_space)
        return int(np.prod(self.env.observation_space.shape)), int(n_acts), int(code)

    def _standardize_scalars(self, critic=False):
        """The host side's standardisation pair: Python scalars, or CPU vectors with per_feature_obs_standardization.
        critic: of critic_obs_stats (its own cache), for the critic's observation rows."""
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

    def _increment_obs_stats(self, obs_dev, critic=False):
        """The host side's statistics increment: WelfordRunningStat.increment(obs, n) on the device (bit-exact with the host class's
        sample-by-sample update in the state's dtype -- float32, or float64 after a checkpoint load -- which costs ~10 ms of Python
        per 4096 samples); the host object stays the owner of the state (checkpoints)."""
        device_stats.increment(self.critic_obs_stats if critic else self.obs_stats, obs_dev)

    def _act(self, fused, t, obs_dev, pair, am, S, acts_tm, logp_tm, to_host):
        """The head's side of step t: S[t] takes the policy-input rows, acts_tm[t] / logp_tm[t] the action (the buffer's float
        encoding) and its log-probability.  fused: policy.step, ONE launch that standardises and pads the raw observations on its
        way; else the rows (already in S[t] after the first step) go through act_padded.  -> (the head's action tensor, acts_tm)."""
        na = self.n_agents
        if fused:
            if acts_tm is None:
                acts_tm = torch.empty((S.shape[0] - 1, na, 1), dtype=torch.float32, device=S.device)
            a, _ = self.policy.step(obs_dev, standardize=pair, rows_out=S[t], actions_f32=acts_tm[t].view(na), logp_out=logp_tm[t],
                                    to_host=to_host, action_mask=am)
            return a, acts_tm
        if t == 0:
            self.policy.arena.stage_obs(obs_dev, pair, out=S[0])
        a, lp = self.policy.act_padded(S[t], action_mask=am)
        a = a.view(na, -1)
        if acts_tm is None:
            acts_tm = torch.empty((S.shape[0] - 1, na, a.shape[1]), dtype=torch.float32, device=S.device)
        acts_tm[t].copy_(a)
        logp_tm[t].copy_(lp)
        return a, acts_tm

    @torch.no_grad()
    def collect_timesteps(self, n):
        """-> ((states, actions, log_probs, rewards, next_states, dones, truncated), metrics, n_collected, seconds):
        device tensors in trajectory-major order; `self.value_input_rows` holds states ++ last next_state contiguously."""
        t1 = time.perf_counter()
        arena, side = self.policy.arena, self._side()
        dev, ld, na = _resolve_device(arena.device), arena.ld_in, self.n_agents
        fused = bool(getattr(self.policy, "fused_step", False))
        T = max(1, -(-int(n) // na))
        N_ = na * T
        side.begin(T, dev)
        S = torch.empty((T + 1, na, ld), dtype=torch.float32, device=dev)     # S[t] = policy-input rows of step t; S[T]: the next collect's
        logp_tm = torch.empty((T, na), dtype=torch.float32, device=dev)
        acts_tm = M = CS = None
        metrics = []
        if self._pending_obs is None:   # first collect: the reset observations are acted on RAW (batched_agent_manager.py:366-384)
            self._pending_obs = (side.upload(self._initial_obs), None)
        obs_dev, pair = self._pending_obs
        if self._initial_mask_pending:  # first collect: the environment's answer after its reset()
            self._initial_mask_pending = False
            self._pending_mask = self._env_mask()
        mask = self._pending_mask
        width = None if mask is None else AM.Layout.of(self.policy).width
        if self.critic_observations:    # CS[0] = the critic's rows the agents act on now; first collect: the reset answer, RAW
            if self.value_net is None:
                raise ValueError("critic_observations: the manager needs the critic (value_net) whose arena stages the rows")
            c_arena = self.value_net.arena
            CS = torch.empty((T + 1, na, c_arena.ld_in), dtype=torch.float32, device=dev)
            if self._critic_next_rows is None:
                c_arena.stage_obs(self._critic_initial, None, out=CS[0])
            else:
                CS[0].copy_(self._critic_next_rows)
        for t in range(T):
            am = None
            if mask is not None:
                if M is None:
                    M = torch.empty((T, na, mask.shape[1]), dtype=torch.int32, device=dev)
                M[t].copy_(mask)
                am = AM.Packed(M[t], width)
            a, acts_tm = self._act(fused, t, obs_dev, pair, am, S, acts_tm, logp_tm, side.to_host)
            step = self.env.step(side.action(a))
            if len(step) == 4:
                (obs, r, d, info), tr = step, None
            else:
                obs, r, d, tr, info = step
            obs_dev = side.observations(t, obs)
            # everything below describes `obs`, the observation of step t + 1; the environment is asked in this order
            if mask is not None:
                mask = self._env_mask()
            if self.collect_metrics_fn is not None:
                metrics.append(self.collect_metrics_fn(info["state"]))
            pair = side.pair()   # fetched BEFORE this step's increment (batched_agent_manager.py:230-235)
            side.record(t, r, d, tr, info, pair)   # the environment's own flags; with them, the final observations of its truncations
            cobs_dev = None
            if CS is not None:   # the critic's observation, with ITS pair before this step's increment
                cobs_dev, cpair = side.upload(self._critic_answer()), side.pair(critic=True)
            if self.standardize_obs:  # same cadence as one worker response per step; both statistics move together
                if self.steps_since_obs_stats_update > self.steps_per_obs_stats_increment:
                    side.increment(obs_dev, cobs_dev)
                    self.steps_since_obs_stats_update = 0
                else:
                    self.steps_since_obs_stats_update += 1
            if CS is not None:
                c_arena.stage_obs(cobs_dev, cpair, out=CS[t + 1])
            if not fused or t == T - 1:
                arena.stage_obs(obs_dev, pair, out=S[t + 1])   # the rows the agents act on next = next_states of this step
        self._pending_obs, self._pending_mask, self._next_rows = (obs_dev, pair), mask, S[T]
        if getattr(self.policy, "noise_mode", None) == "host" and hasattr(self.policy, "prefetch_noise"):
            # the NEXT collect's T draws of the reference's CPU noise stream, produced on the helper threads while the value pass,
            # the GAE scan and PPOLearner.learn run (none of them touches torch's CPU generator; if anything does, the chain is
            # dropped at the next draw: engine.HostExponential)
            self.policy.prefetch_noise(na, T)
        # time-major -> trajectory-major (row a * T + t), once; flat[N_] = next_states[-1], what add_new_experience appends (learner.py:347)
        k = acts_tm.shape[2]
        flat = torch.empty((N_ + 1, ld), dtype=torch.float32, device=dev)
        nxt_flat = torch.empty((N_, ld), dtype=torch.float32, device=dev)
        actions = torch.empty((N_, k), dtype=torch.float32, device=dev)
        small = torch.empty((4, N_), dtype=torch.float32, device=dev)   # log_probs, rewards, dones, truncated (flush rule applied)
        rdt, P, F = side.planes()
        N.check(N.lib().rlppo_rollout_to_trajectory_major(stream_ptr(), ptr(S), ptr(acts_tm), ptr(logp_tm), ptr(rdt), na, T, ld, k, ptr(P), ptr(F),
                                                          ptr(flat), ptr(nxt_flat), ptr(actions), ptr(small[0]), ptr(small[1]), ptr(small[2]),
                                                          ptr(small[3])))
        self.action_mask_rows = None if M is None else AM.Packed(M.transpose(0, 1).reshape(N_, M.shape[2]).contiguous(), width)
        if CS is not None:   # mirrors value_input_rows
            rows = torch.empty((N_ + 1, CS.shape[2]), dtype=torch.float32, device=dev)
            rows[:N_].view(na, T, -1).copy_(CS[:T].transpose(0, 1))
            rows[N_].copy_(CS[T][na - 1])
            self.critic_value_input_rows, self._critic_next_rows = rows, CS[T]
        self.value_input_rows = flat
        self.cumulative_timesteps += N_
        side.finish(nxt_flat, S[T], t1)
        experience = (flat[:N_], actions, small[0], small[1], nxt_flat, small[2], small[3])
        return experience, metrics, N_, time.perf_counter() - t1

    def cleanup(self):
        if self.env is not None and hasattr(self.env, "close"):
            self.env.close()
        self.env = None
