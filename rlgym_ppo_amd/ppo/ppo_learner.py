"""PPOLearner -- drop-in for rlgym_ppo/ppo/ppo_learner.py:10-271 with the update running in librlppo.so.

Same constructor, attributes (`policy`, `value_net`, `policy_optimizer`, `value_optimizer`, `cumulative_model_updates`),
`learn(exp) -> 8-key report`, `save_to` / `load_from` (same four .pt files with stock state_dict layouts).  What changed underneath:

  * one call to rlppo_ppo_minibatch per minibatch replaces ~60 eager ATen launches, 5 H2D copies and 5 .item() syncs
    (ppo_learner.py:139-185); the report statistics accumulate in device doubles and are read back once;
  * the epoch permutation is drawn on the host (bit-identical numpy legacy stream) while the GPU is still busy with the previous
    epoch, and only the index vector crosses PCIe;
  * clip_grad_norm_ + Adam.step() are one fused pass over a flat parameter arena (rlppo_clip_adam);
  * the tail of learn() (ppo_learner.py:213-236: update magnitudes, report means) is ONE launch that writes pinned memory and
    releases a completion word (rlppo_learn_report); nothing is enqueued in front of the first pass that the pass does not need;
  * data-parallel: the minibatch slices of a batch are dealt round-robin to the ranks of the default torch.distributed group and
    ONE RCCL all-reduce of the flat gradient arena precedes clipping -- algebraically the reference's own gradient accumulation
    (ppo_learner.py:134-193) with slice j living on rank j % world.

Everything beyond the reference is opt-in, and with every option off learn() is the reference's update, launch for launch: it makes
the calls it always made.  Four options are trailing keyword arguments ("Options beyond the reference"): per-batch
advantage normalisation, Stable-Baselines3's clipped value loss, a target-KL stop of the optimiser steps and the gradient-norm
limit.  The constructor's parameter list is pinned (the reference's plus those four), so every other choice travels in a
reference parameter or is set after construction:

  * policy_type 1: `act_space_size` may be the nvec of a MultiDiscrete(nvec) action space (a sequence of bin counts; `Learner` has
    `multi_discrete_bins`) instead of its length: an integer keeps the reference's eight heads [3, 3, 3, 3, 3, 2, 2, 2] and its kernels.
  * policy_type 3 is the diagonal-Gaussian head with a learnable log_std (ppo/diag_gaussian_policy.py): `act_space_size` = k action
    dimensions, `continuous_var_range` is ignored, log_std starts at 0 (SB3's default).  Its passes go through
    rlppo_ppo_minibatch_diag, its optimiser step through rlppo_clip_adam_pack2_tail (log_std is the tail of the policy's arena).
  * `set_lr_schedule("adaptive", desired_kl=0.01, lr_bounds=(1e-5, 1e-2))` (ppo/lr_schedule.py) is rsl_rl's
    KL-adaptive learning rate, once per optimiser step: both rates are doubles in device memory, moved by the batch's gate
    (rlppo_kl_gate_lr) and read by its optimiser step (rlppo_clip_adam_pack2_lr) -- no host decision, no added wait.
  * `obs_space_size=ObsSizes(d, d_c)` is the asymmetric actor-critic of rsl_rl / Isaac Lab ("privileged observations");
    `self.critic_obs_space_size` says what was built (None: one size).  The critic is built on d_c inputs (construction order and
    generator use unchanged: a seeded policy has the weights it has without it) and every pass reads the buffer's `critic_states`
    matrix through rlppo_ppo_minibatch_critic: one gather launch for both matrices, no paired launches.  Whenever the buffer holds
    `critic_states` the passes take that entry point; a buffer without them and a critic of another width, or the reverse mismatch,
    is a ValueError before the first pass; update precision "bf16" is refused.
  * `set_value_normalization(True)` is rl_games' `normalize_value`: the critic regresses standardised value
    targets and puts out normalised values.  `self.value_norm` (a ValueNorm) owns the running statistic and the scale every pass
    reads (rlppo_ppo_minibatch_vnorm); the buffer keeps REAL-unit targets.  learn() never moves the statistic (`Learner` does, once per
    iteration; a caller of a bare PPOLearner calls `update_value_norm(targets)`) and no collective is added for data-parallel use:
    replicas see the same targets or are given one state (`value_norm_state()` / `load_value_norm_state()`).
    `set_value_normalization(True, preserve_outputs=True)` adds PopArt's weight-preserving step: the launch that moves the statistic
    rescales the critic's last layer, so its real-unit predictions are what they were (`ValueNorm.update(targets, preserve=critic)`,
    rlppo_value_norm_update_popart).  No collective here either: the step is deterministic, so replicas that feed the same targets
    stay bit-identical; replicas that are handed one state are handed the weights with it.
"""
import ctypes
import os
import time

import numpy as np
import torch

from .. import _native as N
from ..dp import all_reduce_sum, dist_info, fuse_runs, slices_for_rank
from ..engine import Workspace, ptr, require_gpu, stream_ptr
from ..util import action_mask as AM
from . import lr_schedule as LRS
from .continuous_policy import ContinuousPolicy
from .diag_gaussian_policy import DiagGaussianPolicy
from .discrete_policy import DiscreteFF
from .multi_discrete_policy import MultiDiscreteFF, check_bins
from .value_estimator import ValueEstimator


class ObsSizes(object):
    """PPOLearner(obs_space_size=ObsSizes(policy, critic)): the policy's observation size and the critic's own."""

    def __init__(self, policy, critic):
        for name, v in (("policy", policy), ("critic", critic)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
                raise ValueError(f"ObsSizes: {name} observation size must be a positive integer, got {v!r}")
        self.policy, self.critic = int(policy), int(critic)

    def __repr__(self):
        return f"ObsSizes(policy={self.policy}, critic={self.critic})"

MAX_GRAD_NORM = 0.5  # ppo_learner.py:187-190


class ValueNorm(object):
    """The running statistic of the value targets and what the kernels read of it (include/rlppo.h, "[vnorm]").
    state: device double[4] = {count, mean, M2, rejected batches}; scale: device float[4] = {mu, 1/sigma, sigma, 0} with
    sigma = sqrt(M2 / count + 1e-5), {0, 1, 1, 0} while count == 0 (the first iteration runs raw)."""

    def __init__(self, device):
        self.state = torch.zeros(4, dtype=torch.float64, device=device)
        self.scale = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32, device=device)
        self._ws = torch.zeros(N.VALUE_NORM_WS_BYTES, dtype=torch.uint8, device=device)   # zeroed once: every call leaves it armed
        self.arg = N.ValueNormArg()
        self.arg.scale = self.scale.data_ptr()

    def update(self, targets, preserve=None):
        """Advance the statistic with a batch of real-unit value targets (fp32 device tensor) and publish the new scale: one launch,
        no host wait.  A batch with a non-finite entry changes nothing but state[3].

        preserve: a ValueEstimator (one output) whose real-unit predictions are to stay what they are -- PopArt's weight-preserving
        step: the same launch rescales its last Linear's weight and bias for the new scale (rlppo_value_norm_update_popart), and the
        arena's native_epoch is bumped, so the packed, bf16 and x3 images are rebuilt before anything reads them.  An optimiser's
        moments for those parameters are left alone, as in PopArt.  No other network is touched."""
        t = targets.reshape(-1)
        assert t.dtype == torch.float32 and t.device == self.state.device
        if t.numel() == 0:
            return
        t = t.contiguous()
        if preserve is None:
            N.check(N.lib().rlppo_value_norm_update(stream_ptr(), ptr(t), t.numel(), ptr(self.state), ptr(self.scale), ptr(self._ws)))
            return
        arena = getattr(preserve, "arena", None)
        if arena is None or arena.d_out != 1:
            raise ValueError("ValueNorm.update: preserve must be a ValueEstimator with one output, got "
                             f"{type(preserve).__name__}" + ("" if arena is None else f" with {arena.d_out} outputs"))
        assert arena.flat.device == self.state.device
        if not arena.is_bound():
            arena.bind()
        last = arena.linears[-1]
        N.check(N.lib().rlppo_value_norm_update_popart(stream_ptr(), ptr(t), t.numel(), ptr(self.state), ptr(self.scale), ptr(self._ws),
                                                       ptr(last.weight), last.weight.numel(), ptr(last.bias)))
        arena.native_epoch += 1

    def denormalize(self, v):
        """Real-unit values of the critic's normalised outputs (a torch op, for users; the scan does it itself)."""
        return v * self.scale[2] + self.scale[0]

    def state_dict(self):
        """{count, mean, var (population), m2, rejected, scale}: one device-to-host read.  count / mean / var are the portable triple;
        m2 and scale make a round trip exact to the bit."""
        count, mean, m2, rejected = (float(x) for x in self.state.cpu().numpy())
        return {"count": count, "mean": mean, "var": m2 / count if count > 0 else 0.0, "m2": m2, "rejected": rejected,
                "scale": [float(x) for x in self.scale.cpu().numpy()]}

    def load_state_dict(self, d):
        count, mean = float(d["count"]), float(d["mean"])
        if not (count >= 0 and np.isfinite(count) and np.isfinite(mean)):
            raise ValueError(f"value normalisation state: count={count!r}, mean={mean!r}")
        m2 = float(d["m2"]) if "m2" in d else float(d["var"]) * count
        if not (m2 >= 0 and np.isfinite(m2)):
            raise ValueError(f"value normalisation state: M2={m2!r}")
        if "scale" in d:
            scale = [float(x) for x in d["scale"]]
        elif count > 0:   # the kernel's arithmetic: double, rounded once
            sd = float(np.sqrt(np.float64(m2) / np.float64(count) + np.float64(1e-5)))
            scale = [mean, 1.0 / sd, sd, 0.0]
        else:
            scale = [0.0, 1.0, 1.0, 0.0]
        self.state.copy_(torch.tensor([count, mean, m2, float(d.get("rejected", 0.0))], dtype=torch.float64))
        self.scale.copy_(torch.tensor(scale, dtype=torch.float64).to(torch.float32))


class FusedAdam(torch.optim.Adam):
    """torch.optim.Adam whose step() is librlppo's fused clip+Adam kernel on the module's flat arena.  State lives
    in two flat tensors; `state[p]` exposes views of them in the stock layout {step, exp_avg, exp_avg_sq}, so
    state_dict()/load_state_dict() and checkpoints interchange with the reference's optimisers."""

    def __init__(self, module, lr):
        self.arena = module.arena
        super().__init__(list(module.arena.params()), lr=lr)
        a = self.arena
        self.exp_avg = torch.zeros(a.n_flat, dtype=torch.float32, device=a.device)
        self.exp_avg_sq = torch.zeros(a.n_flat, dtype=torch.float32, device=a.device)
        self.gnorm2 = torch.zeros(1, dtype=torch.float64, device=a.device)
        self.step_count = 0
        # lr_schedule="adaptive": this optimiser's rate as ONE device double (PPOLearner lays both side by side, as it does gnorm2);
        # param_groups[0]["lr"] is its host copy -- written to the device at the start of a learn(), read back at its end
        self.lr_word = None

    def _expose_state(self):
        o = 0
        for p in self.param_groups[0]["params"]:
            n = p.numel()
            self.state[p] = {"step": torch.tensor(float(self.step_count)),
                             "exp_avg": self.exp_avg[o:o + n].view(p.shape),
                             "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape)}
            o += n

    def zero_grad(self, set_to_none=True):
        self.arena.grad.zero_()  # keep the .grad views alive: the kernels accumulate into the arena

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        g = self.param_groups[0]
        if not self.arena.is_bound():
            self.arena.bind()
        self.step_count += 1
        b1, b2 = g["betas"]
        N.check(N.lib().rlppo_clip_adam(stream_ptr(), ptr(self.arena.flat), ptr(self.arena.grad), ptr(self.exp_avg),
                                        ptr(self.exp_avg_sq), self.arena.n_flat,
                                        float("inf") if max_norm is None else float(max_norm), float(g["lr"]), float(b1),
                                        float(b2), float(g["eps"]), self.step_count, ptr(self.gnorm2)))
        self.arena.native_epoch += 1

    def fused_descriptor(self, max_norm):
        """rlppo_opt_net of THIS update (advances the step count): one half of rlppo_clip_adam_pack2."""
        g = self.param_groups[0]
        a = self.arena
        if not a.is_bound():
            a.bind()
        self.step_count += 1
        b1, b2 = g["betas"]
        d = N.OptNet()
        d.dims, d.n_layers = ctypes.cast(a.dims_c, ctypes.POINTER(ctypes.c_int32)), a.n_layers
        d.params, d.grads = a.flat.data_ptr(), a.grad.data_ptr()
        d.exp_avg, d.exp_avg_sq = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        d.packed, d.gnorm2 = a.packed.data_ptr(), self.gnorm2.data_ptr()
        d.max_norm = float("inf") if max_norm is None else float(max_norm)
        d.lr, d.beta1, d.beta2, d.eps, d.step = float(g["lr"]), float(b1), float(b2), float(g["eps"]), self.step_count
        return d

    def state_dict(self):
        if self.step_count > 0:
            self._expose_state()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        o, step = 0, 0
        for p in self.param_groups[0]["params"]:
            n = p.numel()
            st = self.state.get(p)
            if st:
                self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                step = int(float(st["step"]))
            o += n
        self.step_count = step
        if step > 0:
            self._expose_state()


class _LearnCall(object):
    """What the steps of one learn() share (PPOLearner.learn_steps): the options in force, what _arm_options made of them, the counts."""
    args = st = runs = gate = adapt = run_gate = lr_dev = None   # the passes' arguments, the stream, this rank's fused runs of a batch; the armed gate
    stride = n_iterations = n_minibatch_iterations = n_passes = 0   # n_passes: this rank's passes (each adds one mean to every report statistic)
    stopped_at, grads_zero = None, False   # target_kl: the batch whose KL stopped this learn() (its step and every later one not applied)

    def __init__(self, learner, rank, world):
        self.rank, self.world, self.gate_values = rank, world, {}   # gate_values: batch -> done value of its gate
        self.stop_on = learner.target_kl is not None        # the host's decision wait and the stop word: target_kl alone
        self.adaptive = learner.lr_schedule == "adaptive"
        self.kl_on = self.stop_on or self.adaptive          # KL armed: the slots, the exchange tail, the gate


class OptimizerBarrierTimeout(RuntimeError):
    """The one-launch optimiser tail's grid barrier gave up; see PPOLearner.learn (the learner has already recovered)."""


class PPOLearner(object):
    def __init__(self, obs_space_size, act_space_size, policy_type, policy_layer_sizes, critic_layer_sizes,
                 continuous_var_range, batch_size, n_epochs, policy_lr, critic_lr, clip_range, ent_coef, mini_batch_size,
                 device, normalize_advantages=False, value_clip_range=None, target_kl=None, max_grad_norm=MAX_GRAD_NORM):
        # act_space_size as a sequence: the nvec of a MultiDiscrete action space (a hyper-parameter like the layer sizes: not
        # checkpoint state); checked before anything needs the GPU
        multi_discrete_bins = None
        if not isinstance(act_space_size, (int, float, np.integer, np.floating)) and np.ndim(act_space_size) > 0:
            if int(policy_type) != 1:
                raise ValueError(f"act_space_size={act_space_size!r}: multi-discrete bins are an option of the multi-discrete policy "
                                 f"(policy_type 1), not of policy_type {policy_type}")
            multi_discrete_bins = check_bins(act_space_size)
            act_space_size = len(multi_discrete_bins)
        # obs_space_size as ObsSizes(policy, critic): a critic with observations of its own (checked at its construction, before
        # anything needs the GPU); an integer is one size for both, as in the reference
        critic_obs_space_size = None
        if isinstance(obs_space_size, ObsSizes):
            obs_space_size, critic_obs_space_size = obs_space_size.policy, obs_space_size.critic
        self.critic_obs_space_size = critic_obs_space_size
        self.device = device
        self._dev = require_gpu(device)
        N.lib()  # fail here, loudly, if the HIP library is missing

        assert batch_size % mini_batch_size == 0, "MINIBATCH SIZE MUST BE AN INTEGER MULTIPLE OF BATCH SIZE"

        obs_space_size = int(obs_space_size)
        self.policy_type = int(policy_type)
        # construction order (policy, then critic) fixes the CPU-generator consumption and therefore the initial
        # weights (ppo_learner.py:34-53)
        if policy_type == 3:   # the diagonal-Gaussian head: k means from the network + a learnable log_std (continuous_var_range unused)
            self.policy = DiagGaussianPolicy(obs_space_size, act_space_size, policy_layer_sizes, device).to(device)
            self._act_dim = int(act_space_size)
        elif policy_type == 2:
            self.policy = ContinuousPolicy(obs_space_size, act_space_size * 2, policy_layer_sizes, device,
                                           var_min=continuous_var_range[0], var_max=continuous_var_range[1]).to(device)
            self._act_dim = int(act_space_size)
        elif policy_type == 1:
            self.policy = MultiDiscreteFF(obs_space_size, policy_layer_sizes, device, bins=multi_discrete_bins).to(device)
            self._act_dim = self.policy.n_heads
        else:
            self.policy = DiscreteFF(obs_space_size, act_space_size, policy_layer_sizes, device).to(device)
            self._act_dim = 1
        self.value_net = ValueEstimator(obs_space_size if critic_obs_space_size is None else critic_obs_space_size, critic_layer_sizes,
                                        device).to(device)
        self.mini_batch_size = mini_batch_size

        self.policy_optimizer = FusedAdam(self.policy, lr=policy_lr)
        self.value_optimizer = FusedAdam(self.value_net, lr=critic_lr)
        # both squared-norm accumulators side by side: rlppo_clip_adam_pack2 then clears them with one fill
        self._gnorm2 = torch.zeros(2, dtype=torch.float64, device=self._dev)
        self.policy_optimizer.gnorm2, self.value_optimizer.gnorm2 = self._gnorm2[0:1], self._gnorm2[1:2]
        # grid-barrier state of the one-launch optimiser tail (include/rlppo.h, RLPPO_OPT_SYNC_BYTES): zeroed once, here
        self._opt_sync = torch.zeros(N.OPT_SYNC_BYTES // 4, dtype=torch.int32, device=self._dev)

        n_pol = sum(p.numel() for p in self.policy.parameters() if p.requires_grad)
        n_val = sum(p.numel() for p in self.value_net.parameters() if p.requires_grad)
        print("Trainable Parameters:")
        print(f"{'Component':<10} {'Count':<10}")
        print("-" * 20)
        print(f"{'Policy':<10} {n_pol:<10}")
        print(f"{'Critic':<10} {n_val:<10}")
        print("-" * 20)
        print(f"{'Total':<10} {n_pol + n_val:<10}")
        print(f"Current Policy Learning Rate: {policy_lr}")
        print(f"Current Critic Learning Rate: {critic_lr}")

        self.n_epochs = n_epochs
        self.batch_size = batch_size
        self.clip_range = clip_range
        self.ent_coef = ent_coef
        self.cumulative_model_updates = 0

        # one contiguous gradient buffer [policy | critic] so that data-parallel needs a single all-reduce
        pa, va = self.policy.arena, self.value_net.arena
        # (+ 2 floats: with target_kl set or the adaptive schedule, the exchanged tensor carries this rank's KL partial of the batch in its tail)
        self._grad_ex = torch.zeros(pa.n_flat + va.n_flat + 2, dtype=torch.float32, device=self._dev)
        self._grad_all = self._grad_ex[:pa.n_flat + va.n_flat]
        pa.grad = self._grad_all[:pa.n_flat]
        va.grad = self._grad_all[pa.n_flat:]
        pa.bind()
        va.bind()
        self._stats = torch.zeros(N.N_STATS, dtype=torch.float64, device=self._dev)
        self._stats_clean = True   # rlppo_learn_report leaves the accumulators zeroed for the next learn()
        # [r6] the tail of learn() as one launch (rlppo_learn_report): the parameters before the first optimiser step (copied behind the
        # first pass's launches, where the copy is free), the kernel's ticket block, its pinned output and completion word
        self._before = (torch.empty_like(pa.flat), torch.empty_like(va.flat))
        self._report_ws = torch.zeros(N.REPORT_WS_BYTES, dtype=torch.uint8, device=self._dev)
        self._report_out = torch.zeros(N.REPORT_OUT_DOUBLES, dtype=torch.float64).pin_memory()
        self._report_done = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._report_out_np, self._report_seq = self._report_out.numpy(), 0
        self._ws = Workspace(self._dev)
        self.n_slots = int(os.environ.get("RLPPO_SLOTS", 1))  # minibatches of a batch kept in flight concurrently
        self._diag_scratch = None  # policy_type 3: one region of rlppo_diag_scratch_bytes per slot (partial sums of the log_std gradient)
        # Minibatch fusion.  The reference sums the gradients of a batch's minibatches, each the MB/B-scaled mean over its
        # rows, before ONE clip + Adam (ppo_learner.py:134-193): the minibatches are independent given the parameters and
        # their sum is the 1/B-scaled sum over all their rows.  They only exist to bound activation memory; with 288 GB of
        # HBM a rank evaluates up to `max_fused_minibatches` CONSECUTIVE minibatches in one pass of rlppo_ppo_minibatch
        # (mb = k MB rows, mb_ratio = k MB / B): the same gradient and the same report means up to fp32 summation order,
        # in launches that are k times larger.  RLPPO_FUSE=1 keeps one pass per minibatch.
        self.max_fused_minibatches = max(1, int(os.environ.get("RLPPO_FUSE", 8)))
        self.fused_optimizer_step = os.environ.get("RLPPO_FUSED_OPT", "1") != "0"  # rlppo_clip_adam_pack2 (False: FusedAdam.step x2)
        self.grad_probe = None  # callable(flat [grad_policy | grad_value]) before every optimiser step (tests)
        self.one_launch_optimizer = os.environ.get("RLPPO_OPT_ONE_LAUNCH", "1") != "0"  # ... as ONE launch with a grid barrier
        # [r5] update precision of THIS learner (rlppo_minibatch_args.precision): None = the process default chosen with
        # engine.set_update_precision, else "fp32" / "bf16" / "x3" -- two learners of one process may differ
        self.update_precision = None
        # options beyond the reference (plain attributes, read by every learn(); None / False = the reference's update)
        self.normalize_advantages = normalize_advantages
        self.value_clip_range = value_clip_range
        self.target_kl = target_kl
        self.max_grad_norm = max_grad_norm
        self._opt = None      # their device state, allocated on first use
        self._kl_seq = 0
        # learning-rate schedule (plain attributes like the options above, read by every learn(); set_lr_schedule checks and sets
        # them at once).  "adaptive": [policy rate, critic rate, KL_b of the last gate (written only while lr_probe is set)] in
        # device doubles + the pinned pair the rates come back in with the report
        self.lr_schedule, self.desired_kl, self.lr_bounds = "constant", 0.01, (1e-5, 1e-2)
        self.report_learning_rates = False   # (Learner sets it for its "linear" schedule)
        self.lr_probe = None  # callable(rates [2] device doubles {policy, critic}, KL_b [1] device double) after every gate (tests)
        self._lr_dev = self._lr_host = None
        self.value_norm = None   # set_value_normalization(True): a ValueNorm; None = the critic regresses raw value targets
        self.value_norm_preserve_outputs = False   # set_value_normalization(True, preserve_outputs=True): PopArt's weight-preserving step

    def set_value_normalization(self, on=True, preserve_outputs=False):
        """Train the critic on standardised value targets from now on (module docstring), or stop doing so.  Switching it on keeps a
        statistic that exists; a fresh one publishes {0, 1, 1, 0}: raw until its first update.  preserve_outputs (the attribute
        value_norm_preserve_outputs): update_value_norm rescales the critic's last layer with every move of the statistic."""
        if preserve_outputs and not on:
            raise ValueError("set_value_normalization: preserve_outputs=True needs on=True (there is no statistic to move with the option off)")
        self.value_norm_preserve_outputs = bool(preserve_outputs)
        if not on:
            self.value_norm = None
        elif self.value_norm is None:
            self.value_norm = ValueNorm(self._dev)

    def update_value_norm(self, targets):
        """Advance the statistic with a batch of real-unit value targets: ValueNorm.update, with this learner's critic as `preserve`
        where value_norm_preserve_outputs is set.  Never part of learn(); checkpoint loads and load_value_norm_state never rescale."""
        if self.value_norm is None:
            raise ValueError("update_value_norm: value normalisation is off (set_value_normalization(True) first)")
        self.value_norm.update(targets, preserve=self.value_net if self.value_norm_preserve_outputs else None)

    def value_norm_state(self):
        """The statistic as a dictionary (ValueNorm.state_dict), None with the option off: what a replica or a checkpoint needs."""
        return None if self.value_norm is None else self.value_norm.state_dict()

    def load_value_norm_state(self, state):
        if self.value_norm is None:
            raise ValueError("load_value_norm_state: value normalisation is off (set_value_normalization(True) first)")
        self.value_norm.load_state_dict(state)

    # --------------------------------------------------------------------------------------------- learn
    def _minibatch_args(self, exp, rank=0, world=1):
        pa, va = self.policy.arena, self.value_net.arena
        a = N.MinibatchArgs()
        a.head = self.policy_type
        a.pol_layers, a.val_layers = pa.n_layers, va.n_layers
        a.act_dim = self._act_dim
        a.pol_dims = ctypes.cast(pa.dims_c, ctypes.POINTER(ctypes.c_int32))
        a.val_dims = ctypes.cast(va.dims_c, ctypes.POINTER(ctypes.c_int32))
        a.pol_packed, a.val_packed = pa.packed.data_ptr(), va.packed.data_ptr()
        prec = {"fp32": 0, "bf16": 1, "x3": 2}[self._precision()]
        a.precision = N.PRECISION_DEFAULT if self.update_precision is None else 1 + prec
        self._bf16 = prec == 1  # bf16-operand forward: the rounded weight images travel too
        self._x3 = prec == 2    # [r4] fp32 update with split-bf16 hidden forward / dX products: the three-plane images travel
        if self._x3:
            a.pol_wb16, a.val_wb16 = pa.ensure_packed_x3().data_ptr(), va.ensure_packed_x3().data_ptr()
        if self._bf16:
            (pr, pw), (vr, vw) = pa.ensure_packed_bf16(), va.ensure_packed_bf16()
            a.pol_packed_r, a.val_packed_r, a.pol_wb16, a.val_wb16 = pr.data_ptr(), vr.data_ptr(), pw.data_ptr(), vw.data_ptr()
        a.pol_grad, a.val_grad = pa.grad.data_ptr(), va.grad.data_ptr()
        st, a.ring_base, a.ring_cap = exp.ring()  # physical rows; the kernels map the permutation's logical rows onto them
        a.states, a.ld_states, a.n_rows = st["states"].data_ptr(), st["states"].shape[1], st["states"].shape[0]
        a.actions, a.old_logp = st["actions"].data_ptr(), st["log_probs"].data_ptr()
        a.targets, a.advantages = st["values"].data_ptr(), st["advantages"].data_ptr()
        if "action_masks" in st:  # invalid-action masking (ExperienceBuffer.submit_experience(..., action_masks=...))
            lay = self.policy.mask_layout
            if lay is None:
                raise ValueError(f"the experience buffer holds action masks: {AM.REFUSAL}, not of policy_type {self.policy_type}")
            if exp.mask_width != lay.width:  # (the C side sees the word count only: 33 and 40 entries are two words alike)
                raise ValueError(f"the experience buffer's action masks have {exp.mask_width} entries per row, the "
                                 + (f"multi-discrete policy has {lay.width} logits (one entry per bin of every component)"
                                    if lay.heads is not None else f"discrete policy has {lay.width} actions"))
            a.action_mask, a.mask_words = st["action_masks"].data_ptr(), st["action_masks"].shape[1]
        # the critic's own rows (ExperienceBuffer.submit_experience(..., critic_states=...)): rlppo_ppo_minibatch_critic
        cr = None
        d_c = getattr(exp, "critic_width", None)
        if d_c is None and va.d_in != pa.d_in:
            raise ValueError(f"the critic observes {va.d_in} features and the policy {pa.d_in} (ObsSizes), but the experience "
                             "buffer holds no critic_states: submit_experience(..., critic_states=...)")
        if d_c is not None:
            if d_c != va.d_in:
                raise ValueError(f"the experience buffer's critic_states have {d_c} features, the critic observes {va.d_in}"
                                 + ("" if self.critic_obs_space_size is not None else " (PPOLearner was built without ObsSizes)"))
            cr = N.CriticRows()
            cr.states, cr.ld_states = st["critic_states"].data_ptr(), st["critic_states"].shape[1]
        a.clip_range, a.ent_coef = float(self.clip_range), float(self.ent_coef)
        a.mb_ratio = float(self.mini_batch_size / self.batch_size)
        if self.policy_type == 2:
            a.var_m, a.var_b = float(self.policy.affine_map.m), float(self.policy.affine_map.b)
        a.stats = self._stats.data_ptr()
        # one activation workspace per slot: minibatches in different slots overlap on the GPU (rlppo_ppo_join)
        # rows of the largest pass THIS rank launches: its share of a batch's slices, fused (8 ranks x 8 slices: one 65,536-row pass)
        n_slices = self.batch_size // self.mini_batch_size
        runs = fuse_runs(slices_for_rank(max(1, n_slices), rank, world), self.max_fused_minibatches)
        self._fused_rows = self.mini_batch_size * max([cnt for _, cnt in runs] or [1])
        size_fn = N.lib().rlppo_minibatch_workspace_bytes_for if cr is None else N.lib().rlppo_minibatch_workspace_bytes_critic
        nbytes = int(size_fn(pa.dims_c, pa.n_layers, va.dims_c, va.n_layers, self._fused_rows, a.precision))
        nbytes = (nbytes + 255) // 256 * 256
        ws = self._ws.get(nbytes * self.n_slots)
        self._slot_ws = [ws.data_ptr() + i * nbytes for i in range(self.n_slots)]
        a.workspace, a.ws_bytes = self._slot_ws[0], nbytes
        if self.policy_type == 3:   # allocated once per slot (grown only when a larger pass comes)
            sb = (int(N.lib().rlppo_diag_scratch_bytes(self._fused_rows, self._act_dim)) + 255) // 256 * 256
            if self._diag_scratch is None or self._diag_scratch.numel() < sb * self.n_slots:
                self._diag_scratch = torch.empty(sb * self.n_slots, dtype=torch.uint8, device=self._dev)
            self._diag_scratch_bytes = sb
        a.call = self._pass_call(a, cr)   # (a Python attribute of the ctypes struct: the choice travels with the arguments it was made for)
        return a

    def _pass_call(self, args, crit=None):
        """How a learn()'s passes are called, decided once -> (entry point, its arguments behind (stream, args), ext, scratch base, crit).
        The entry point: value normalisation, else critic rows, else _ex for a tanh / ELU network (LayerSizes), else the head's own form (_diag;
        _nvec for bins of its own and for every masked pass, which runs the general loss kernel also on the reference's bins; else the plain
        one).  The head's parts are written once, into the ext every form takes them from."""
        L, pa, va, vn = N.lib(), self.policy.arena, self.value_net.arena, self.value_norm
        e, scratch = N.MinibatchExt(), 0
        e.pol_hidden_act, e.val_hidden_act = pa.hidden_act, va.hidden_act
        if self.policy_type == 3:   # log_std and its gradient: the tail of the policy's arena, behind the layers; one scratch region per slot
            e.log_std, e.log_std_grad = pa.flat.data_ptr() + 4 * pa.n_net, pa.grad.data_ptr() + 4 * pa.n_net
            scratch, e.scratch_bytes = self._diag_scratch.data_ptr(), self._diag_scratch_bytes
        elif self.policy_type == 1 and (self.policy.md_nvec is not None or args.action_mask):
            e.md_nvec, e.md_heads = ctypes.cast(self.policy._nvec_c, ctypes.POINTER(ctypes.c_int32)), self.policy.n_heads
        if vn is not None:      # the value loss reads the targets through the statistic's scale
            fn, tail = L.rlppo_ppo_minibatch_vnorm, (ctypes.byref(e), None if crit is None else ctypes.byref(crit), ctypes.byref(vn.arg))
        elif crit is not None:  # the buffer holds critic_states: the critic reads its own matrix
            fn, tail = L.rlppo_ppo_minibatch_critic, (ctypes.byref(e), ctypes.byref(crit))
        elif pa.hidden_act or va.hidden_act:
            fn, tail = L.rlppo_ppo_minibatch_ex, (ctypes.byref(e),)
        elif self.policy_type == 3:
            fn, tail = L.rlppo_ppo_minibatch_diag, None   # (the ext's four diag fields, read per pass: the scratch moves with the slot)
        elif e.md_nvec:
            fn, tail = L.rlppo_ppo_minibatch_nvec, (e.md_nvec, e.md_heads)
        else:
            fn, tail = L.rlppo_ppo_minibatch, ()
        return fn, tail, e, scratch, crit

    def _pass(self, st, args):
        """One pass of the update through the entry point _minibatch_args chose for these arguments."""
        fn, tail, e, scratch, _ = getattr(args, "call", None) or self._pass_call(args)
        if scratch:
            e.scratch = scratch + args.slot * e.scratch_bytes
        return fn(st, ctypes.byref(args), *((e.log_std, e.log_std_grad, e.scratch, e.scratch_bytes) if tail is None else tail))

    _ADAPTIVE_NEEDS_FUSED = ("lr_schedule='adaptive' needs the library's optimiser step (RLPPO_FUSED_OPT=1): the FusedAdam.step form takes "
                             "its rate from the host and cannot read one the gate wrote on the device")

    def set_lr_schedule(self, lr_schedule="constant", desired_kl=0.01, lr_bounds=(1e-5, 1e-2)):
        """Choose the learning-rate schedule of every later learn(): "constant" (the default: the update as it was, launch for
        launch) or "adaptive" (module docstring).  Checked here, on the host alone -- a ValueError leaves the learner as it was;
        the rates "adaptive" starts from are the optimisers' current ones (param_groups[0]["lr"])."""
        self.lr_schedule, self.desired_kl, self.lr_bounds = self._checked_schedule(lr_schedule, desired_kl, lr_bounds)
        self.report_learning_rates = self.lr_schedule != "constant"

    def _checked_schedule(self, lr_schedule, desired_kl, lr_bounds):
        checked = LRS.check_schedule(lr_schedule, desired_kl, lr_bounds, policy_lr=self.policy_optimizer.param_groups[0]["lr"],
                                     critic_lr=self.value_optimizer.param_groups[0]["lr"], allow_linear=False)
        if checked[0] == "adaptive" and not self.fused_optimizer_step:
            raise ValueError(self._ADAPTIVE_NEEDS_FUSED)
        return checked

    def _precision(self):
        """The update precision of this learner's passes by name: its own, else the process default."""
        return self.update_precision or ("fp32", "bf16", "x3")[int(N.lib().rlppo_get_update_precision())]

    def _check_options(self, exp=None):
        # separate critic rows update in fp32 or x3: the bf16 gather writes one bf16 image, of the policy's rows
        critic_rows = getattr(self, "critic_obs_space_size", None) is not None or (exp is not None and getattr(exp, "critic_width", None) is not None)
        if critic_rows and self._precision() == "bf16":
            raise ValueError("update_precision='bf16' with separate critic observations (ObsSizes / critic_states): the "
                             "bf16 gather writes one bf16 image, of the policy's rows -- use 'fp32' or 'x3'")
        # a tanh / ELU network updates in fp32: the bf16 and split-bf16 kernels carry the ReLU bitmask by construction
        acts = {m.hidden_activation for m in (self.policy, self.value_net)} - {"relu"}
        prec = self._precision() if acts else "fp32"
        if prec != "fp32":
            raise ValueError(f"hidden activation {sorted(acts)[0]!r} with update precision {prec!r}: the {prec} update kernels are ReLU "
                             "only -- use update_precision='fp32'")
        self.lr_schedule, self.desired_kl, self.lr_bounds = self._checked_schedule(self.lr_schedule, self.desired_kl, self.lr_bounds)
        if self.value_clip_range is not None and not float(self.value_clip_range) > 0:
            raise ValueError(f"value_clip_range must be > 0 or None, got {self.value_clip_range!r}")
        if self.target_kl is not None and not float(self.target_kl) > 0:
            raise ValueError(f"target_kl must be > 0 or None, got {self.target_kl!r}")
        if self.max_grad_norm is None or not float(self.max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm must be > 0, got {self.max_grad_norm!r}")
        if self.target_kl is not None and not self.fused_optimizer_step:
            raise ValueError("target_kl needs the library's optimiser step (RLPPO_FUSED_OPT=1): the FusedAdam.step form cannot skip a step "
                             "on the device")

    def _option_state(self, kl_slot_doubles=0):
        """Device buffers of the options: advantage statistics {mean, scale} + their ticket block, the stop word, the KL slots,
        pinned decision words (4 batches x {stop, done})."""
        if self._opt is None:
            self._opt = dict(adv=torch.zeros(2, dtype=torch.float32, device=self._dev),
                             adv_ws=torch.zeros(N.ADV_STATS_WS_BYTES, dtype=torch.uint8, device=self._dev),
                             stop=torch.zeros(1, dtype=torch.int32, device=self._dev),
                             kl=torch.zeros(0, dtype=torch.float64, device=self._dev),
                             host=torch.zeros(8, dtype=torch.int32).pin_memory())
            self._opt["host_np"] = self._opt["host"].numpy().view(np.uint32)
        o = self._opt
        if o["kl"].numel() < kl_slot_doubles:
            o["kl"] = torch.zeros(kl_slot_doubles, dtype=torch.float64, device=self._dev)
        return o

    def _lr_state(self):
        """Device doubles of the adaptive schedule, refreshed from the optimisers' host copies (a rate written to
        param_groups[0]["lr"] between two learn() calls is honoured): two fills, scalars as launch arguments -- no copy, no wait."""
        if self._lr_dev is None:
            self._lr_dev = torch.zeros(3, dtype=torch.float64, device=self._dev)
            self._lr_host = torch.zeros(2, dtype=torch.float64).pin_memory()
            self.policy_optimizer.lr_word, self.value_optimizer.lr_word = self._lr_dev[0:1], self._lr_dev[1:2]
        for opt in (self.policy_optimizer, self.value_optimizer):
            opt.lr_word.fill_(float(opt.param_groups[0]["lr"]))
        return self._lr_dev

    def _wait_word(self, address, value, what):
        """Wait for `value` in the pinned word at `address`: a short spin, then once more behind the stream (a long learn(): sleep
        instead of spinning); RuntimeError(what) if it still has not arrived."""
        L = N.lib()
        if L.rlppo_host_wait_words(address, 1, value, 5000) != 0:
            torch.cuda.current_stream(self._dev).synchronize()
            if L.rlppo_host_wait_words(address, 1, value, 1000000) != 0:
                raise RuntimeError(what)

    def _kl_decision(self, c, g):
        """Waits for the pinned words of batch g's gate; a stop word (0 = running, else trigger + 1) sets c.stopped_at.  -> stopped"""
        self._wait_word(self._opt["host"].data_ptr() + 8 * (g % 4) + 4, c.gate_values[g], "rlppo_kl_gate: the decision word did not arrive")
        v = int(self._opt["host_np"][2 * (g % 4)])
        c.stopped_at = v - 1 if v else None
        return v != 0

    def learn(self, exp):
        """Compute PPO updates with an experience buffer; returns the reference's report dictionary
        (ppo_learner.py:225-234)."""
        dist, rank, world = dist_info()
        steps = self.learn_steps(exp, rank, world)
        try:
            buf = next(steps)
            while True:  # one exchange per optimiser step + one for the report statistics (dp.py)
                all_reduce_sum(buf, dist)
                buf = steps.send(None)
        except StopIteration as done:
            return done.value

    def learn_steps(self, exp, rank=0, world=1):
        """learn() as a generator that stops at every data-parallel exchange point: it yields the flat tensor whose sum over the
        ranks it needs (the [grad_policy | grad_value] arena after a batch's last backward pass, the report statistics at the end)
        and continues once the caller has put that sum into it; the report dictionary is the generator's return value.  learn()
        drives it with torch.distributed's all-reduce; dp.run_virtual_ranks drives the generators of N replicas in ONE process
        (the 8-way partition of BASELINE configs[3] on a one-GPU box).  With world == 1 it never yields.  What its steps share is `c`."""
        L = N.lib()
        self._check_options(exp)
        pa, va = self.policy.arena, self.value_net.arena
        B, MB = self.batch_size, self.mini_batch_size
        n_slices = B // MB
        c = _LearnCall(self, rank, world)
        # [r6] nothing is enqueued before the first pass that the pass does not need: the previous learn()'s report kernel zeroed the report
        # sums, and the "before" copies of the parameters (ppo_learner.py:111-116) follow the first pass's launches (the first step is behind them)
        if not self._stats_clean:
            self._stats.zero_()
        self._stats_clean = False
        have_before = False
        total = len(exp)
        n_batches = total // B if B > 0 else 0
        t1 = time.time()
        if n_batches > 0 and total > 0:
            if exp.ring()[0]["actions"][:1].reshape(1, -1).shape[1] != self._act_dim:
                raise ValueError("experience buffer action width does not match the policy head")
            args = c.args = self._minibatch_args(exp, rank, world)
            st = c.st = stream_ptr()
            runs = c.runs = fuse_runs(slices_for_rank(n_slices, rank, world), self.max_fused_minibatches)
            self._arm_options(c)
            # The legacy-MT19937 permutation is serial host work: the buffer's shuffle pipeline draws it on helper threads several
            # epochs ahead (also across learn() calls) and uploads every index vector on its own stream (engine.LegacyPermutation /
            # DeviceIndexRing), so here an epoch only orders the stream after that copy.
            for epoch in range(self.n_epochs):
                if c.stopped_at is not None:   # a stopped learn() still consumes every epoch's permutation
                    exp.epoch_indices()
                    continue
                idx_dev = exp.epoch_indices_device(refill=False)   # (the look-ahead is topped up behind the epoch's first launches)
                refilled = False
                for b in range(n_batches):
                    g = epoch * n_batches + b
                    # at most one undecided batch beyond the executing one: batch g waits for the decision of batch g - 2
                    if c.stop_on and g >= 2 and self._kl_decision(c, g - 2):
                        break
                    if not c.grads_zero:
                        self._grad_all.zero_()
                    c.grads_zero = False
                    pa.ensure_packed()
                    va.ensure_packed()
                    if self._bf16:  # re-round the master weights the optimiser step just moved (one small launch per net)
                        pa.ensure_packed_bf16()
                        va.ensure_packed_bf16()
                    if self._x3:    # re-split them (two small launches per covered layer)
                        pa.ensure_packed_x3()
                        va.ensure_packed_x3()
                    if self.normalize_advantages:   # mean and 1 / (std + 1e-8) of this batch's advantages, before its first pass
                        N.check(L.rlppo_adv_stats(st, idx_dev.data_ptr() + 8 * b * B, B, args.advantages, args.ring_base, args.ring_cap,
                                                  args.adv_norm, self._opt["adv_ws"].data_ptr()))
                    for k, (j, cnt) in enumerate(runs):
                        if c.kl_on:
                            args.kl_slots = c.gate.kl_slots + 8 * k * c.stride
                        args.slot = k % self.n_slots
                        args.workspace = self._slot_ws[args.slot]
                        args.idx = idx_dev.data_ptr() + 8 * (b * B + j * MB)
                        args.mb = cnt * MB                      # cnt consecutive minibatches in one pass
                        args.mb_ratio = float(cnt * MB / B)
                        N.check(self._pass(st, args))
                        c.n_passes += 1
                    N.check(L.rlppo_ppo_join(st))
                    if not refilled:
                        exp.refill_shuffle()
                        refilled = True
                    if not have_before:
                        self._before[0].copy_(pa.flat)
                        self._before[1].copy_(va.flat)
                        have_before = True
                    c.n_minibatch_iterations += n_slices
                    if c.stop_on:
                        self._kl_seq = self._kl_seq % 0x7FFFFFFF + 1
                        c.gate_values[g] = self._kl_seq
                        c.gate.batch, c.gate.done_value = g, self._kl_seq
                        c.gate.host_words = self._opt["host"].data_ptr() + 8 * (g % 4)
                    if c.kl_on and world > 1:  # this rank's KL share rides in the tail of the ONE exchange of the step
                        c.gate.phase = 1
                        N.check(c.run_gate())
                    if world > 1:
                        yield self._grad_ex if c.kl_on else self._grad_all  # summed over the ranks (RCCL over xGMI) before clipping
                    if c.kl_on:
                        c.gate.phase = 2 if world > 1 else 0
                        if c.adaptive:
                            c.adapt.kl_out = c.lr_dev.data_ptr() + 16 if self.lr_probe is not None else None
                        N.check(c.run_gate())
                        if c.adaptive and self.lr_probe is not None:  # test hook: the rates this batch's step will use, the KL that set them
                            self.lr_probe(c.lr_dev[:2], c.lr_dev[2:3])
                    if self.grad_probe is not None:  # test hook: the batch gradient clip_grad_norm_ / Adam are about to see
                        self.grad_probe(self._grad_all)
                    self._optimizer_step(c)
                    c.n_iterations += 1
                if not refilled:
                    exp.refill_shuffle()
            if c.stop_on:
                self._settle_stop(c, n_slices)
        else:
            for _ in range(self.n_epochs):
                exp.epoch_indices()  # the reference consumes one permutation per epoch even if no batch fits
        if not have_before:   # (no batch fitted: nothing moved)
            self._before[0].copy_(pa.flat)
            self._before[1].copy_(va.flat)
        return (yield from self._report(c, t1, lr_back=c.adaptive and self._lr_dev is not None and n_batches > 0 and total > 0))

    def _arm_options(self, c):
        """The options into c.args, their device state, and with KL armed the gate (+ adapt) struct and c.run_gate."""
        L, args, st = N.lib(), c.args, c.st
        if self.value_clip_range is not None:
            args.value_clip = float(self.value_clip_range)
        if not (self.normalize_advantages or c.kl_on):
            return
        c.stride = int(L.rlppo_kl_slots_doubles(self._fused_rows))
        o = self._option_state(c.stride * max(len(c.runs), 1) if c.kl_on else 0)
        if self.normalize_advantages:
            args.adv_norm = o["adv"].data_ptr()
        if c.kl_on:
            gate = c.gate = N.KlGateArgs()
            gate.kl_slots, gate.slot_stride, gate.n_passes = o["kl"].data_ptr(), c.stride, len(c.runs)
            gate.exchange = self._grad_ex.data_ptr() + 4 * self._grad_all.numel()
            c.run_gate = lambda: L.rlppo_kl_gate(st, ctypes.byref(gate))
        if c.stop_on:
            o["stop"].zero_()
            args.stop_word = gate.stop_word = o["stop"].data_ptr()
            gate.threshold = 1.5 * float(self.target_kl)
        if c.adaptive:   # the gate moves the two rates, the optimiser step reads them: the host takes no part until the report
            c.lr_dev = self._lr_state()
            adapt = c.adapt = N.LrAdaptArgs()
            adapt.lr, adapt.n_lr, adapt.desired_kl, adapt.factor = c.lr_dev.data_ptr(), 2, self.desired_kl, LRS.ADAPT_FACTOR
            adapt.lr_min, adapt.lr_max = self.lr_bounds
            c.run_gate = lambda: L.rlppo_kl_gate_lr(st, ctypes.byref(gate), ctypes.byref(adapt))

    def _optimizer_step(self, c):
        """clip + Adam of both networks: FusedAdam.step twice (RLPPO_FUSED_OPT=0), or the library's form -- both steps, the re-pack of
        both weight copies and the next batch's zero_grad in 3 stream operations instead of 9 (csrc/optim.hip)."""
        L, pa, va, max_norm = N.lib(), self.policy.arena, self.value_net.arena, float(self.max_grad_norm)
        if not self.fused_optimizer_step:
            self.value_optimizer.step(max_norm=max_norm)
            self.policy_optimizer.step(max_norm=max_norm)
            return
        dv, dp_ = self.value_optimizer.fused_descriptor(max_norm), self.policy_optimizer.fused_descriptor(max_norm)
        if c.stop_on:   # (a step after the stop touches nothing: the gate's stop word)
            dv.skip_word = dp_.skip_word = c.gate.stop_word
        call = (c.st, ctypes.byref(dv), ctypes.byref(dp_), ptr(self._opt_sync) if self.one_launch_optimizer else None)
        if c.adaptive:   # both rates from the device doubles the gate has just left (descriptor order: critic, policy)
            rc = L.rlppo_clip_adam_pack2_lr(*call, va.n_tail, pa.n_tail, self.value_optimizer.lr_word.data_ptr(),
                                            self.policy_optimizer.lr_word.data_ptr())
        elif va.n_tail or pa.n_tail:   # parameters behind a network's layers (log_std): same norm, same step, never packed
            rc = L.rlppo_clip_adam_pack2_tail(*call, va.n_tail, pa.n_tail)
        else:
            rc = L.rlppo_clip_adam_pack2(*call)
        N.check(rc)
        va.mark_repacked()
        pa.mark_repacked()
        c.grads_zero = True

    def _settle_stop(self, c, n_slices):
        """target_kl, behind the last batch: the outstanding decision, and after a stop the counts of what was applied."""
        if c.stopped_at is None and c.n_iterations > 0:   # a trigger among the last two batches
            self._kl_decision(c, c.n_iterations - 1)
        if c.stopped_at is None:
            return
        # launches from the trigger on were skipped on the device: Adam's step counts rewind by them (as after a give-up),
        # the gradient arena holds the unapplied batches' sums, and only the evaluated batches' passes are in the report
        for opt in (self.policy_optimizer, self.value_optimizer):
            opt.step_count -= c.n_iterations - c.stopped_at
        c.n_iterations = c.stopped_at
        c.n_passes = len(c.runs) * (c.stopped_at + 1)
        c.n_minibatch_iterations = n_slices * (c.stopped_at + 1)
        self._grad_all.zero_()
        c.grads_zero = True

    def _report(self, c, t1, lr_back):
        """[r6] update magnitudes (ppo_learner.py:214-222), the statistics and the give-up words in ONE launch that writes pinned
        memory and releases a completion word (rlppo_learn_report): one device->host hand-over per learn(), no eager tail.
        A sub-generator (the statistics' exchange, the recovery's) -> the report dictionary."""
        pa, va = self.policy.arena, self.value_net.arena
        rep = N.ReportArgs()
        rep.pol_before, rep.pol_now, rep.n_pol = self._before[0].data_ptr(), pa.flat.data_ptr(), pa.n_flat
        rep.val_before, rep.val_now, rep.n_val = self._before[1].data_ptr(), va.flat.data_ptr(), va.n_flat
        # every pass added one mean to each report statistic; the number of passes travels with the sums, so the report is the
        # mean over the passes of ALL ranks even when the slices do not divide evenly over them (3 slices on 2 ranks)
        rep.stats, rep.add_passes = self._stats.data_ptr(), float(c.n_passes)
        rep.timeout_word = self._opt_sync.data_ptr() + 4 * N.OPT_SYNC_TIMEOUT_WORD   # optimiser steps THIS rank's barrier skipped
        if c.world > 1:
            # the give-up count travels with the statistics: a give-up on ANY rank is known to EVERY rank after this exchange
            self._stats[N.STAT_PASSES] += float(c.n_passes)
            rep.add_passes = 0.0
            ex = torch.cat((self._stats, self._opt_sync[N.OPT_SYNC_TIMEOUT_WORD:N.OPT_SYNC_TIMEOUT_WORD + 1].double()))
            yield ex
            self._stats.copy_(ex[:N.N_STATS])
            to_all = ex[N.N_STATS:].contiguous()
            rep.extra = to_all.data_ptr()
        if lr_back:   # the two rates ride to pinned memory in front of the report launch: its completion word covers them too
            self._lr_host.copy_(self._lr_dev[:2], non_blocking=True)
        self._report_seq = self._report_seq % 0x7FFFFFFF + 1
        rep.out, rep.done_word, rep.ws, rep.done_value = self._report_out.data_ptr(), self._report_done.data_ptr(), self._report_ws.data_ptr(), self._report_seq
        N.check(N.lib().rlppo_learn_report(stream_ptr(), ctypes.byref(rep)))
        self._wait_word(self._report_done.data_ptr(), self._report_seq, "rlppo_learn_report: the completion word did not arrive")
        self._stats_clean = True
        stats = self._report_out_np.copy()
        if lr_back:   # gate state, not step state: they stand whatever became of the steps (stopped, skipped, given up)
            self.policy_optimizer.param_groups[0]["lr"], self.value_optimizer.param_groups[0]["lr"] = (float(x) for x in self._lr_host.numpy())
        if stats[N.N_STATS + 3] != 0:
            yield from self._recover_barrier_timeout(c, stats)
        elapsed, n_iter_r, n_mb_r = time.time() - t1, max(c.n_iterations, 1), max(float(stats[N.STAT_PASSES]), 1.0)
        self.cumulative_model_updates += c.n_iterations if c.stop_on else n_iter_r   # (with target_kl: applied steps only)
        report = {
            "PPO Batch Consumption Time": elapsed / n_iter_r,
            "Cumulative Model Updates": self.cumulative_model_updates,
            "Policy Entropy": float(stats[N.STAT_ENTROPY]) / n_mb_r,
            "Mean KL Divergence": float(stats[N.STAT_KL]) / n_mb_r,
            "Value Function Loss": float(stats[N.STAT_VLOSS]) / n_mb_r,
            "SB3 Clip Fraction": float(stats[N.STAT_CLIPFRAC]) / n_mb_r if c.n_minibatch_iterations else 0,
            "Policy Update Magnitude": float(stats[N.N_STATS]),
            "Value Function Update Magnitude": float(stats[N.N_STATS + 1]),
        }
        if c.stop_on:
            report["PPO Optimizer Steps"] = c.n_iterations
            report["KL Early Stopped"] = 1.0 if c.stopped_at is not None else 0.0
        if self.report_learning_rates:   # the optimisers' rates after this learn() ("adaptive": as its last gate left them; "linear": this iteration's)
            report["Policy Learning Rate"] = float(self.policy_optimizer.param_groups[0]["lr"])
            report["Critic Learning Rate"] = float(self.value_optimizer.param_groups[0]["lr"])
        if not c.grads_zero:  # the fused optimiser step leaves the arena zeroed
            self._grad_all.zero_()
        return report

    def _recover_barrier_timeout(self, c, stats):
        """A grid-barrier wait of the one-launch optimiser step gave up on some rank (GPU shared with a kernel that never yields, a partitioned
        device, or a defect).  Giving up is all or nothing (include/rlppo.h): on the rank it happened, that step and every later one of this
        call were SKIPPED -- parameters and Adam moments are those of its last completed step, finite -- and its gradient arena holds the
        skipped batches' sums.  Recovers a state to continue from (zero gradients, a re-armed block, the three-operation form) and raises."""
        pa, va = self.policy.arena, self.value_net.arena
        opts = (self.policy_optimizer, self.value_optimizer)
        n_to = int(stats[N.N_STATS + 2])   # skipped optimiser steps of THIS rank (a launch counts itself once: csrc/optim.hip)
        for opt in opts:
            opt.step_count = max(0, opt.step_count - n_to)   # Adam's bias corrections must not count steps that never happened
        self.cumulative_model_updates += max(0, c.n_iterations - n_to)
        self._grad_all.zero_()
        self._opt_sync.zero_()
        self.one_launch_optimizer = False
        where = "the affected optimiser steps of this learn() were skipped -- parameters and Adam state are those of the last completed step, no NaN was written"
        if c.world > 1:
            # [r5, advisor] Data-parallel: the rank that gave up skipped steps the others applied, so the replicas have DIVERGED (parameters,
            # moments, step counts).  The outcome is made collective: every rank takes this branch (the count was summed over the ranks) and
            # adopts rank 0's state -- one more exchange in which only rank 0 contributes, so the sum IS its state -- before raising.
            pieces = [pa.flat, va.flat] + [t for o in opts for t in (o.exp_avg, o.exp_avg_sq)]
            sync = torch.cat([t.reshape(-1) for t in pieces])
            counts = torch.tensor([float(o.step_count) for o in opts] + [float(self.cumulative_model_updates)], dtype=torch.float64,
                                  device=self._dev)
            if c.rank != 0:
                sync.zero_()
                counts.zero_()
            yield sync
            yield counts
            off = 0
            for t in pieces:
                t.copy_(sync[off:off + t.numel()].view_as(t))
                off += t.numel()
            n = counts.cpu().numpy()
            self.policy_optimizer.step_count, self.value_optimizer.step_count = int(n[0]), int(n[1])
            self.cumulative_model_updates = int(n[2])
            pa.native_epoch += 1  # `flat` was rewritten behind torch's back: re-pack before the next kernel reads the weights
            va.native_epoch += 1
            pa.invalidate()
            va.invalidate()
            where = ("the rank(s) it happened on skipped optimiser steps the others applied; every rank has now adopted rank 0's "
                     "parameters, Adam moments and step counts (bit-identical replicas again), no NaN was written")
        raise OptimizerBarrierTimeout(
            "rlppo_clip_adam_pack2: the optimiser's grid barrier gave up (%d skipped step(s) over all ranks); %s -- gradients are "
            "zeroed and this learner now uses the three-operation optimiser tail: calling learn() again is safe"
            % (int(stats[N.N_STATS + 3]), where))

    # ---------------------------------------------------------------------------------------- checkpoints
    def save_to(self, folder_path):
        os.makedirs(folder_path, exist_ok=True)
        torch.save(self.policy.state_dict(), os.path.join(folder_path, "PPO_POLICY.pt"))
        torch.save(self.value_net.state_dict(), os.path.join(folder_path, "PPO_VALUE_NET.pt"))
        torch.save(self.policy_optimizer.state_dict(), os.path.join(folder_path, "PPO_POLICY_OPTIMIZER.pt"))
        torch.save(self.value_optimizer.state_dict(), os.path.join(folder_path, "PPO_VALUE_NET_OPTIMIZER.pt"))

    def load_from(self, folder_path):
        assert os.path.exists(folder_path), "PPO LEARNER CANNOT FIND FOLDER {}".format(folder_path)
        self.policy.load_state_dict(torch.load(os.path.join(folder_path, "PPO_POLICY.pt")))
        self.value_net.load_state_dict(torch.load(os.path.join(folder_path, "PPO_VALUE_NET.pt")))
        self.policy_optimizer.load_state_dict(torch.load(os.path.join(folder_path, "PPO_POLICY_OPTIMIZER.pt")))
        self.value_optimizer.load_state_dict(torch.load(os.path.join(folder_path, "PPO_VALUE_NET_OPTIMIZER.pt")))
