"""Learner -- drop-in for rlgym_ppo.Learner (reference: rlgym_ppo/learner.py:28-576).

Same 40 constructor parameters, same loop (collect -> add_new_experience -> PPOLearner.learn -> report -> checkpoint),
same checkpoint folder layout and BOOK_KEEPING_VARS.json.  The three hot calls of the loop body (learner.py:257-270)
run on the GPU through librlppo.so: rollout inference inside BatchedAgentManager._send_actions, value pass + GAE in
add_new_experience (device-resident, no tolist()), and the PPO update.
"""
import json
import os
import random
import shutil
import time
import warnings

import numpy as np
import torch

from .batched_agents import BatchedAgentManager, VectorAgentManager
from .ppo import ExperienceBuffer, PPOLearner
from .util import KBHit, WelfordRunningStat, reporting, torch_functions

try:  # wandb is optional (not installed on the build/GPU boxes)
    import wandb
except ImportError:  # pragma: no cover
    wandb = None


class Learner(object):
    def __init__(
            self, env_create_function, metrics_logger=None, n_proc: int = 8, min_inference_size: int = 80,
            render: bool = False, render_delay: float = 0,
            timestep_limit: int = 5_000_000_000, exp_buffer_size: int = 100000, ts_per_iteration: int = 50000,
            standardize_returns: bool = True, standardize_obs: bool = True, max_returns_per_stats_increment: int = 150,
            steps_per_obs_stats_increment: int = 5,
            policy_layer_sizes=(256, 256, 256), critic_layer_sizes=(256, 256, 256), continuous_var_range=(0.1, 1.0),
            ppo_epochs: int = 10, ppo_batch_size: int = 50000, ppo_minibatch_size=None, ppo_ent_coef: float = 0.005,
            ppo_clip_range: float = 0.2, gae_lambda: float = 0.95, gae_gamma: float = 0.99, policy_lr: float = 3e-4,
            critic_lr: float = 3e-4,
            log_to_wandb: bool = False, load_wandb: bool = True, wandb_run=None, wandb_project_name=None,
            wandb_group_name=None, wandb_run_name=None,
            checkpoints_save_folder=None, add_unix_timestamp: bool = True, checkpoint_load_folder="latest",
            save_every_ts: int = 1_000_000, instance_launch_delay=None, random_seed: int = 123,
            n_checkpoints_to_keep: int = 5, shm_buffer_size: int = 8192, device: str = "auto",
            vector_env: bool = False, gae_bootstrap_truncated: bool = False, multi_discrete_bins=None,
            continuous_head: str = "reference", continuous_log_std_init: float = 0.0, continuous_action_clip="default",
            hidden_activation: str = "relu",
            ppo_lr_schedule: str = "constant", ppo_desired_kl: float = 0.01, ppo_lr_bounds=(1e-5, 1e-2),
            critic_observations: bool = False,
            ppo_normalize_value: bool = False, ppo_value_norm_popart: bool = False,
            per_feature_obs_standardization: bool = False,
            ppo_normalize_advantages: bool = False, ppo_value_clip_range=None, ppo_target_kl=None, ppo_max_grad_norm: float = 0.5):
        assert env_create_function is not None, "MUST PROVIDE A FUNCTION TO CREATE RLGYM FUNCTIONS TO INITIALIZE RLGYM-PPO"
        # not in the reference: continuous_head="diag" is the diagonal-Gaussian head with a learnable log_std (ppo/diag_gaussian_policy.py)
        # for a continuous action space; "reference" (default) keeps ContinuousPolicy.  The head samples unbounded actions and the buffer
        # stores them unclipped; continuous_action_clip = (lo, hi) is what the ENVIRONMENT receives ("default": (-1, 1) with "diag", the
        # range the reference's head clamps to; None: no clipping).  The option values are checked here, before anything needs the GPU
        # or spawns a process; that the action space IS continuous can only be checked once the environment has reported it (below,
        # before the PPOLearner is built -- like multi_discrete_bins).
        # not in the reference: the learning-rate schedule (ppo/lr_schedule.py) -- "adaptive" is PPOLearner's (decided on the device, per
        # optimiser step); "linear" is this loop's: before every learn() both rates are lr0 * max(0, 1 - T / timestep_limit), T the
        # cumulative timesteps before the iteration's collect (stateless: a loaded checkpoint derives them from its book-keeping)
        # not in the reference (whose networks are ReLU): hidden_activation = "relu" | "tanh" | "elu" (alpha = 1) for every hidden layer of
        # the policy AND the critic.  It travels to the networks inside the layer sizes (ppo.LayerSizes); sizes that already are a
        # LayerSizes keep their activation while hidden_activation is left at its default and must agree with it otherwise.  Checked
        # here, before anything is built or spawned.  (The default IS "relu", so an explicit hidden_activation="relu" cannot be told
        # from an omitted one: LayerSizes(..., "tanh") beside it builds a tanh network and raises nothing -- the one disagreement that
        # is not refused.  self.hidden_activations says what was built.)
        # not in the reference: critic_observations=True is the asymmetric actor-critic of rsl_rl / Isaac Lab ("privileged observations") --
        # the vector environment's critic_observations() -> [n_agents, d_c] describes, for the critic alone, the state the agents act on
        # next; the critic is built on d_c inputs (taken from the first answer), the value pass and the update read those rows
        # (VectorAgentManager.critic_value_input_rows, ExperienceBuffer.critic_states).  Vector mode only: the process-mode wire format
        # has no slot for the rows; and not together with gae_bootstrap_truncated, which would need FINAL critic observations.  Checked
        # here, before anything is built or spawned; False is the library as it was, launch for launch.
        # not in the reference: ppo_value_norm_popart=True adds PopArt's weight-preserving step to ppo_normalize_value -- the launch that
        # advances the statistic rescales the critic's last layer, so the critic's real-unit predictions are not moved by the
        # book-keeping.  An option of ppo_normalize_value; checked here, before anything is built or spawned.
        if ppo_value_norm_popart and not ppo_normalize_value:
            raise ValueError("ppo_value_norm_popart=True needs ppo_normalize_value=True: there is no running statistic whose moves "
                             "the critic's last layer could follow")
        self.critic_observations = bool(critic_observations)
        if self.critic_observations:
            if not vector_env:
                raise ValueError("critic_observations=True needs vector_env=True: process-mode collection is not supported (its wire format "
                                 "has no slot for the critic's observation rows)")
            if gae_bootstrap_truncated:
                raise ValueError("critic_observations=True together with gae_bootstrap_truncated=True is not supported: bootstrapping a "
                                 "truncated step needs the critic's FINAL observation of the episode, which the environment interface "
                                 "does not carry yet")
        from .ppo._mlp import LayerSizes, check_activation
        hidden_activation = check_activation(hidden_activation)

        def with_activation(name, sizes):
            own = getattr(sizes, "activation", None)
            if own is not None and own != hidden_activation and hidden_activation != "relu":
                raise ValueError(f"{name} is LayerSizes(..., {own!r}) but hidden_activation={hidden_activation!r}: give one of them")
            return LayerSizes(sizes, own if own is not None else hidden_activation)
        sizes_given = (policy_layer_sizes, critic_layer_sizes)   # (what the config dict logs, as it always did)
        policy_layer_sizes = with_activation("policy_layer_sizes", policy_layer_sizes)
        critic_layer_sizes = with_activation("critic_layer_sizes", critic_layer_sizes)
        # what was built, per network; and as one name where both agree (the keyword's own type), None where they differ
        self.hidden_activations = {"policy": policy_layer_sizes.activation, "critic": critic_layer_sizes.activation}
        self.hidden_activation = policy_layer_sizes.activation if policy_layer_sizes.activation == critic_layer_sizes.activation else None
        from .ppo import lr_schedule as LRS
        ppo_lr_schedule, ppo_desired_kl, ppo_lr_bounds = LRS.check_schedule(ppo_lr_schedule, ppo_desired_kl, ppo_lr_bounds,
                                                                            policy_lr=policy_lr, critic_lr=critic_lr)
        if ppo_lr_schedule == "linear" and not (timestep_limit is not None and timestep_limit > 0):
            raise ValueError(f"ppo_lr_schedule='linear' needs timestep_limit > 0, got {timestep_limit!r}")
        if ppo_lr_schedule == "adaptive" and os.environ.get("RLPPO_FUSED_OPT", "1") == "0":   # (here: nothing is spawned yet)
            raise ValueError(PPOLearner._ADAPTIVE_NEEDS_FUSED)
        self.lr_schedule, self._lr0 = ppo_lr_schedule, [policy_lr, critic_lr]
        if continuous_head not in ("reference", "diag"):
            raise ValueError(f"continuous_head must be 'reference' or 'diag', got {continuous_head!r}")
        from .ppo.diag_gaussian_policy import check_log_std_init
        from .util.action_clip import ClippedEnvFactory, check_clip
        continuous_log_std_init = check_log_std_init(continuous_log_std_init)
        default_clip = isinstance(continuous_action_clip, str) and continuous_action_clip == "default"   # (a pair may be an array)
        if continuous_head == "reference":
            if not default_clip:
                raise ValueError("continuous_action_clip is an option of continuous_head='diag': the reference's head clamps its own "
                                 f"samples to [-1, 1] (got {continuous_action_clip!r})")
            continuous_action_clip = None
        else:
            continuous_action_clip = check_clip((-1.0, 1.0) if default_clip else continuous_action_clip)
            if continuous_action_clip is not None:   # one mechanism for both collection modes: the environment is built wrapped
                env_create_function = ClippedEnvFactory(env_create_function, *continuous_action_clip)
        self.continuous_head, self.continuous_action_clip = continuous_head, continuous_action_clip
        if checkpoints_save_folder is None:
            checkpoints_save_folder = os.path.join("data", "checkpoints", "rlgym-ppo-run")
        self.add_unix_timestamp = add_unix_timestamp
        if add_unix_timestamp:
            checkpoints_save_folder = f"{checkpoints_save_folder}-{time.time_ns()}"

        torch.manual_seed(random_seed)
        np.random.seed(random_seed)
        random.seed(random_seed)

        self.n_checkpoints_to_keep = n_checkpoints_to_keep
        self.checkpoints_save_folder = checkpoints_save_folder
        self.max_returns_per_stats_increment = max_returns_per_stats_increment
        self.metrics_logger = metrics_logger
        self.standardize_returns = standardize_returns
        self.save_every_ts = save_every_ts
        self.ts_since_last_save = 0

        if device in {"auto", "gpu"}:
            if not torch.cuda.is_available():
                raise RuntimeError("rlgym_ppo_amd.Learner needs an AMD GPU visible to PyTorch (no CPU fallback)")
            self.device = f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}"
        else:
            self.device = device
        torch.cuda.set_device(torch.device(self.device))
        print(f"Using device {self.device}")

        self.exp_buffer_size = exp_buffer_size
        self.timestep_limit = timestep_limit
        self.ts_per_epoch = ts_per_iteration
        self.gae_lambda = gae_lambda
        self.gae_gamma = gae_gamma
        self.return_stats = WelfordRunningStat(1)
        self.epoch = 0
        # construction order buffer -> manager -> processes -> PPOLearner fixes RNG consumption (learner.py:124-167)
        self.experience_buffer = ExperienceBuffer(self.exp_buffer_size, seed=random_seed, device=self.device)

        print("Initializing processes...")
        collect_metrics_fn = None if metrics_logger is None else self.metrics_logger.collect_metrics
        # vector_env=True (not in the reference): env_create_function builds ONE vectorised environment whose agents step in
        # lockstep; the rollout then stays on the GPU (batched_agents/vector_agent_manager.py)
        manager_cls = VectorAgentManager if vector_env else BatchedAgentManager
        self.agent = manager_cls(None, min_inference_size=min_inference_size, seed=random_seed,
                                 standardize_obs=standardize_obs,
                                 steps_per_obs_stats_increment=steps_per_obs_stats_increment)
        # not in the reference (which standardises every feature with the statistics of feature 0, quirk Q5): every feature
        # with its own running mean / std
        self.agent.per_feature_obs_standardization = bool(per_feature_obs_standardization)
        # not in the reference (quirk Q3: a truncated step bootstraps from values[step + 1], the first state of whichever trajectory
        # follows in concatenation order): bootstrap it from V of its own next state, as SB3 / CleanRL / Gymnasium's time limits do
        self.gae_bootstrap_truncated = bool(gae_bootstrap_truncated)
        if vector_env:
            self.agent.bootstrap_truncated = self.gae_bootstrap_truncated
            self.agent.critic_observations = self.critic_observations   # (init_processes refuses an environment without the method)
        obs_space_size, act_space_size, action_space_type = self.agent.init_processes(
            n_processes=n_proc, build_env_fn=env_create_function, collect_metrics_fn=collect_metrics_fn,
            spawn_delay=instance_launch_delay, render=render, render_delay=render_delay, shm_buffer_size=shm_buffer_size)
        obs_space_size = np.prod(obs_space_size)
        print("Initializing PPO...")
        if ppo_minibatch_size is None:
            ppo_minibatch_size = ppo_batch_size
        if multi_discrete_bins is not None:   # the nvec of the environment's MultiDiscrete space (PPOLearner takes it as act_space_size)
            from .ppo.multi_discrete_policy import check_bins
            if action_space_type != 1:
                raise ValueError(f"multi_discrete_bins is an option of the multi-discrete policy (action space type 1), not of type {action_space_type}")
            multi_discrete_bins = check_bins(multi_discrete_bins)
            if len(multi_discrete_bins) != int(act_space_size):
                raise ValueError(f"multi_discrete_bins has {len(multi_discrete_bins)} entries, but the action space has "
                                 f"{int(act_space_size)} components")
            act_space_size = multi_discrete_bins
        if continuous_head == "diag":
            if action_space_type != 2:
                self.agent.cleanup()
                raise ValueError(f"continuous_head='diag' is an option of a continuous action space (type 2), not of action space type {action_space_type}")
            action_space_type = 3   # PPOLearner's policy_type of the diagonal-Gaussian head
        if self.critic_observations:   # the critic's input size is the environment's first answer (ppo.ObsSizes carries both sizes)
            from .ppo import ObsSizes
            obs_space_size = ObsSizes(int(obs_space_size), self.agent.critic_obs_size)
        self.ppo_learner = PPOLearner(
            obs_space_size, act_space_size, device=self.device, batch_size=ppo_batch_size,
            mini_batch_size=ppo_minibatch_size, n_epochs=ppo_epochs, continuous_var_range=continuous_var_range,
            policy_type=action_space_type, policy_layer_sizes=policy_layer_sizes, critic_layer_sizes=critic_layer_sizes,
            policy_lr=policy_lr, critic_lr=critic_lr, clip_range=ppo_clip_range, ent_coef=ppo_ent_coef,
            normalize_advantages=ppo_normalize_advantages, value_clip_range=ppo_value_clip_range, target_kl=ppo_target_kl,
            max_grad_norm=ppo_max_grad_norm)
        if self.critic_observations:
            self.agent.value_net = self.ppo_learner.value_net   # its arena stages the critic's observation rows
        # not in the reference: ppo_normalize_value trains the critic on standardised value targets (rl_games' normalize_value;
        # PPOLearner.set_value_normalization).  The statistic is checkpoint state (value_norm_running_stats in the book).
        self.normalize_value = bool(ppo_normalize_value)
        self._value_norm_host = None   # (mu, sigma, rejected batches) as of the last add_new_experience: its one read-back
        self.value_norm_popart = bool(ppo_value_norm_popart)
        if self.normalize_value:
            self.ppo_learner.set_value_normalization(True, preserve_outputs=self.value_norm_popart)
        if ppo_lr_schedule == "adaptive":   # ("linear" is this loop's: the update runs the constant schedule's launches)
            self.ppo_learner.set_lr_schedule("adaptive", ppo_desired_kl, ppo_lr_bounds)
        self.ppo_learner.report_learning_rates = ppo_lr_schedule != "constant"
        if continuous_head == "diag":   # (a constant fill before the first step and before a checkpoint is loaded: no generator use)
            self.ppo_learner.policy.fill_log_std(continuous_log_std_init)
        self.agent.policy = self.ppo_learner.policy
        if not vector_env and self.agent.masked:
            # a masked MultiDiscrete environment: its masks' width against the policy's bins, here rather than at the first collect
            try:
                self.agent._mask_layout()
            except ValueError:
                self.agent.cleanup()
                raise
        # not in the reference (whose multi-discrete policy has eight fixed heads): multi_discrete_bins is the environment's nvec.
        # It is never taken from the environment by itself -- the default stays the reference's policy -- but where the
        # environment is in this process (vector mode) a disagreement is worth one warning.
        nvec = getattr(getattr(getattr(self.agent, "env", None), "action_space", None), "nvec", None) if vector_env else None
        if action_space_type == 1 and nvec is not None:
            in_effect = [int(b) for b in self.ppo_learner.policy.splits]
            if [int(b) for b in np.asarray(nvec).reshape(-1)] != in_effect:
                warnings.warn(f"the environment's action space is MultiDiscrete({list(np.asarray(nvec).reshape(-1))}) but the policy samples "
                              f"bins {in_effect}: pass multi_discrete_bins to Learner", RuntimeWarning, stacklevel=2)

        self.config = {
            "n_proc": n_proc, "min_inference_size": min_inference_size, "timestep_limit": timestep_limit,
            "exp_buffer_size": exp_buffer_size, "ts_per_iteration": ts_per_iteration,
            "standardize_returns": standardize_returns, "standardize_obs": standardize_obs,
            "policy_layer_sizes": sizes_given[0], "critic_layer_sizes": sizes_given[1], "ppo_epochs": ppo_epochs,
            # (a hyper-parameter like the layer sizes, not checkpoint state)
            "hidden_activation": self.hidden_activation if self.hidden_activation is not None else dict(self.hidden_activations),
            "ppo_batch_size": ppo_batch_size, "ppo_minibatch_size": ppo_minibatch_size, "ppo_ent_coef": ppo_ent_coef,
            "ppo_clip_range": ppo_clip_range, "gae_lambda": gae_lambda, "gae_gamma": gae_gamma, "policy_lr": policy_lr,
            "critic_lr": critic_lr, "shm_buffer_size": shm_buffer_size,
            "gae_bootstrap_truncated": self.gae_bootstrap_truncated,  # (a hyper-parameter, not checkpoint state)
            "critic_observations": self.critic_observations,
            "ppo_normalize_value": self.normalize_value, "ppo_value_norm_popart": self.value_norm_popart,
        }

        self.wandb_run = wandb_run
        # "adaptive": the rates are run state -- a checkpoint's optimisers carry them (param_groups), the constructor's start a fresh run
        # only; "linear": recomputed before every learn() anyway
        lrs = (None, None) if ppo_lr_schedule != "constant" else (policy_lr, critic_lr)
        wandb_loaded = checkpoint_load_folder is not None and self.load(checkpoint_load_folder, load_wandb, *lrs)
        if log_to_wandb and self.wandb_run is None and not wandb_loaded:
            if wandb is None:
                raise RuntimeError("log_to_wandb=True but the wandb package is not installed")
            self.wandb_run = wandb.init(project=wandb_project_name or "rlgym-ppo", group=wandb_group_name or "unnamed-runs",
                                        config=self.config, name=wandb_run_name or "rlgym-ppo-run", reinit=True)
            print("Created new wandb run!", self.wandb_run.id)
        print("Learner successfully initialized!")

    def update_learning_rate(self, new_policy_lr=None, new_critic_lr=None):
        # ("adaptive": the schedule goes on from the new rate at the next learn(); "linear": the new rate is the one annealed from)
        if new_policy_lr is not None:
            self.policy_lr = self._lr0[0] = new_policy_lr
            for group in self.ppo_learner.policy_optimizer.param_groups:
                group["lr"] = new_policy_lr
            print(f"New policy learning rate: {new_policy_lr}")
        if new_critic_lr is not None:
            self.critic_lr = self._lr0[1] = new_critic_lr
            for group in self.ppo_learner.value_optimizer.param_groups:
                group["lr"] = new_critic_lr
            print(f"New critic learning rate: {new_critic_lr}")

    def learn(self):
        """Run the loop; on any error print it, try to checkpoint, always clean up (learner.py:218-238)."""
        try:
            self._learn()
        except Exception:
            import traceback
            print("\n\nLEARNING LOOP ENCOUNTERED AN ERROR\n")
            traceback.print_exc()
            try:
                self.save(self.agent.cumulative_timesteps)
            except Exception:
                print("FAILED TO SAVE ON EXIT")
        finally:
            self.cleanup()

    def _learn(self):
        kb = KBHit()
        print("Press (p) to pause (c) to checkpoint, (q) to checkpoint and quit (after next iteration)\n")
        while self.agent.cumulative_timesteps < self.timestep_limit:
            epoch_start = time.perf_counter()
            if self.lr_schedule == "linear":
                from .ppo.lr_schedule import linear_lr
                for opt, lr0 in zip((self.ppo_learner.policy_optimizer, self.ppo_learner.value_optimizer), self._lr0):
                    opt.param_groups[0]["lr"] = linear_lr(lr0, self.agent.cumulative_timesteps, self.timestep_limit)
            experience, collected_metrics, steps_collected, collection_time = self.agent.collect_timesteps(self.ts_per_epoch)
            if self.metrics_logger is not None:
                self.metrics_logger.report_metrics(collected_metrics, self.wandb_run, self.agent.cumulative_timesteps)
            self.add_new_experience(experience)
            report = dict(self.ppo_learner.learn(self.experience_buffer))
            epoch_time = time.perf_counter() - epoch_start
            if self.epoch < 1:
                report["Value Function Loss"] = np.nan  # quirk Q10
            report["Cumulative Timesteps"] = self.agent.cumulative_timesteps
            report["Total Iteration Time"] = epoch_time
            report["Timesteps Collected"] = steps_collected
            report["Timestep Collection Time"] = collection_time
            report["Timestep Consumption Time"] = epoch_time - collection_time
            report["Collected Steps per Second"] = steps_collected / collection_time
            report["Overall Steps per Second"] = steps_collected / epoch_time
            report["Policy Reward"] = self.agent.average_reward if self.agent.average_reward is not None else np.nan
            if self.normalize_value and self._value_norm_host is not None:   # ("Value Function Loss" is in normalised units then)
                report["Value Norm Mean"], report["Value Norm Std"] = self._value_norm_host[0], self._value_norm_host[1]
            self.ts_since_last_save += steps_collected
            reporting.report_metrics(loggable_metrics=report, debug_metrics=None, wandb_run=self.wandb_run)

            if kb.kbhit():
                c = kb.getch()
                if c == "p":
                    print("Paused, press any key to resume")
                    while not kb.kbhit():
                        time.sleep(0.05)
                if c in ("c", "q"):
                    self.save(self.agent.cumulative_timesteps)
                if c == "q":
                    return
                if c in ("c", "p"):
                    print("Resuming...\n")
            if self.ts_since_last_save >= self.save_every_ts:
                self.save(self.agent.cumulative_timesteps)
                self.ts_since_last_save = 0
            self.epoch += 1

    @torch.no_grad()
    def add_new_experience(self, experience):
        """Value pass on [N+1, d] (states + the last next_state, learner.py:347-349), GAE, return statistics, buffer
        submit -- all on the device; only min(150, N) returns come back to the host (learner.py:368-372).

        gae_bootstrap_truncated: the m steps that are truncated and not done (known from the HOST copies of the flags: no
        read-back) get V of their own next state -- process mode: m more rows in the one value pass; vector mode: a value pass
        on the manager's m next-state rows -- scattered into a length-N device buffer for the bootstrap form of the scan.  A
        device-resident vector environment (the manager's bootstrap_dense): the flags exist on the device only, so one value pass over
        all N next-state rows gives the dense boot_values as they are.

        ppo_normalize_value: the value pass yields NORMALISED values; the scan takes every one of them (bootstrap values included) to
        real units under the statistic as it stands -- the one the critic was trained under -- so targets, advantages and returns are
        in real units as always; then the statistic advances with this call's N value targets (one launch) and learn() runs under
        the new, fixed scale.  mu, sigma and the count of rejected batches ride in the call's one device-to-host read.
        ppo_value_norm_popart: that one launch also rescales the critic's last layer for the new scale (PPOLearner.update_value_norm),
        so learn() starts from a critic whose real-unit predictions are the ones the scan just used; the order of steps is the same."""
        states, actions, log_probs, rewards, next_states, dones, truncated = experience
        value_net = self.ppo_learner.value_net
        n = states.shape[0]
        on_device = isinstance(states, torch.Tensor) and states.is_cuda   # VectorAgentManager: rollout already in HBM
        boot_values = boot_idx = dense_boot = None
        if on_device:
            rows = self.agent.value_input_rows               # [N+1, ld]: states ++ the last next_state, padded
            assert rows.shape[0] == n + 1 and rows.data_ptr() == states.data_ptr()
            d_logical = int(self.ppo_learner.policy.arena.d_in)
            critic_rows = self.agent.critic_value_input_rows if self.critic_observations else None   # [N+1, ld_c]: the critic's own rows
            if critic_rows is not None:
                assert critic_rows.shape[0] == n + 1
            val_preds = value_net.forward_padded(rows if critic_rows is None else critic_rows).contiguous()
            if self.gae_bootstrap_truncated and getattr(self.agent, "bootstrap_dense", False):
                # a device-resident environment: which steps are truncated is known on the device only -- one value pass over ALL N
                # next-state rows; the scan selects by the flags and never uses the other entries (include/rlppo.h, rlppo_gae_boot)
                dense_boot = value_net.forward_padded(self.agent.bootstrap_rows).contiguous()
            elif self.gae_bootstrap_truncated and self.agent.bootstrap_steps.size:
                boot_idx = self.agent.bootstrap_index        # None: exactly the last step of every agent (the flush)
                boot_values = value_net.forward_padded(self.agent.bootstrap_rows)
        else:
            flat_states = np.asarray(states).reshape(n, -1)
            parts = [flat_states, np.asarray(next_states[-1]).reshape(1, -1)]
            if self.gae_bootstrap_truncated:
                steps = np.flatnonzero((np.asarray(truncated).reshape(n) != 0) & (np.asarray(dones).reshape(n) == 0))
                if steps.size:
                    parts.append(np.asarray(next_states).reshape(n, -1)[steps])
                    boot_idx = steps
            val_inp = np.concatenate(parts, axis=0)
            rows = value_net.arena.stage_obs(val_inp)        # zero-padded fp32 device rows [N+1 (+m), ld]
            d_logical = int(flat_states.shape[1])
            val_preds = value_net.forward_padded(rows).contiguous()
            if boot_idx is not None:
                boot_values, val_preds = val_preds[n + 1:], val_preds[:n + 1]
                boot_idx = torch.from_numpy(boot_idx).to(rows.device)
                rows = rows[:n + 1]

        dev = rows.device
        if boot_values is not None:   # scatter the m values to their steps; the other entries are never used (include/rlppo.h)
            m, boot = boot_values.shape[0], torch.empty(n, dtype=torch.float32, device=dev)
            if boot_idx is None:
                boot.view(m, n // m)[:, -1] = boot_values
            else:
                boot[boot_idx] = boot_values
            boot_values = boot
        elif dense_boot is not None:
            boot_values = dense_boot
        up = lambda x: x.to(dev, torch.float32) if isinstance(x, torch.Tensor) else \
            torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to(dev)
        rews_d, dones_d, trunc_d = up(rewards), up(dones), up(truncated)
        ret_std = self.return_stats.std[0] if self.standardize_returns else None
        value_norm = self.ppo_learner.value_norm if self.normalize_value else None
        gae_kw = {} if boot_values is None else {"boot_values": boot_values}
        if value_norm is not None:
            gae_kw["value_scale"] = value_norm.scale
        value_targets, advantages, returns, gae_timeouts = torch_functions.gae_device_deferred(
            rews_d, dones_d, trunc_d, val_preds, gamma=self.gae_gamma, lmbda=self.gae_lambda, return_std=ret_std, **gae_kw)
        if value_norm is not None:   # (ppo_value_norm_popart: the same launch rescales the critic's last layer for the new scale)
            self.ppo_learner.update_value_norm(value_targets)

        # ONE device-to-host read per call: the scan's timeout counter travels with the min(150, N) returns the statistics need
        n_to_increment = min(self.max_returns_per_stats_increment, n) if self.standardize_returns else 0
        parts = [returns[:n_to_increment]] + ([gae_timeouts.float()] if gae_timeouts is not None else [])
        n_head = n_to_increment + (1 if gae_timeouts is not None else 0)
        if value_norm is not None:   # mu, sigma, rejected batches (a count: exact in float32 far beyond any run)
            parts += [value_norm.scale[0:1], value_norm.scale[2:3], value_norm.state[3:4].float()]
        host = torch.cat(parts).cpu().numpy()
        if gae_timeouts is not None:
            torch_functions.raise_if_timed_out(host[n_head - 1])   # GAETimeout: NaN advantages must never reach the buffer
        if value_norm is not None:
            before = self._value_norm_host[2] if self._value_norm_host is not None else 0.0
            self._value_norm_host = tuple(float(x) for x in host[n_head:n_head + 3])
            if self._value_norm_host[2] > before:
                warnings.warn("value normalisation: this iteration's value targets are not all finite -- the batch was left out of the "
                              "running statistic", RuntimeWarning, stacklevel=2)
        if self.standardize_returns:
            head = host[:n_to_increment]
            if np.isnan(head).any():
                raise RuntimeError("GAE produced NaN returns (NaN inputs): refusing to train on them")
            self.return_stats.increment(head, n_to_increment)

        self.experience_buffer._d = d_logical  # logical width of the padded rows
        extra = {}
        if on_device and self.critic_observations:
            self.experience_buffer._dc = int(value_net.arena.d_in)
            extra["critic_states"] = critic_rows[:n]
        # invalid-action masking (an environment with action_masks(), either collection mode): the masks the actions were sampled
        # under -- packed device words from the vector manager, bool host rows [N, n_actions] from process-mode collection
        masks = getattr(self.agent, "action_mask_rows", None)
        if masks is not None:
            self.experience_buffer.submit_experience(rows[:n], actions, log_probs, rews_d, next_states, dones_d, trunc_d,
                                                     value_targets, advantages, action_masks=masks, **extra)
            return
        self.experience_buffer.submit_experience(rows[:n], actions, log_probs, rews_d, next_states, dones_d, trunc_d,
                                                 value_targets, advantages, **extra)

    # ------------------------------------------------------------------------------------------ checkpoints
    def save(self, cumulative_timesteps):
        from .dp import dist_info
        if dist_info()[1] != 0:
            return  # data-parallel replicas are bit-identical: rank 0 writes the checkpoint
        folder_path = os.path.join(self.checkpoints_save_folder, str(cumulative_timesteps))
        os.makedirs(folder_path, exist_ok=True)
        print(f"Saving checkpoint {cumulative_timesteps}...")
        existing = sorted(int(name) for name in os.listdir(self.checkpoints_save_folder) if name.isdigit())
        if len(existing) > self.n_checkpoints_to_keep:
            for name in existing[:-self.n_checkpoints_to_keep]:
                shutil.rmtree(os.path.join(self.checkpoints_save_folder, str(name)))
        os.makedirs(folder_path, exist_ok=True)
        self.ppo_learner.save_to(folder_path)
        book = {
            "cumulative_timesteps": self.agent.cumulative_timesteps,
            "cumulative_model_updates": self.ppo_learner.cumulative_model_updates,
            "policy_average_reward": self.agent.average_reward,
            "epoch": self.epoch,
            "ts_since_last_save": self.ts_since_last_save,
            "reward_running_stats": self.return_stats.to_json(),
        }
        if self.agent.standardize_obs and self.agent.obs_stats is not None:
            book["obs_running_stats"] = self.agent.obs_stats.to_json()
        if self.critic_observations and self.agent.standardize_obs and getattr(self.agent, "critic_obs_stats", None) is not None:
            book["critic_obs_running_stats"] = self.agent.critic_obs_stats.to_json()
        if getattr(self, "normalize_value", False):   # count / mean / var (+ what makes the round trip exact to the bit)
            book["value_norm_running_stats"] = self.ppo_learner.value_norm_state()
        if self.wandb_run is not None:
            book.update(wandb_run_id=self.wandb_run.id, wandb_project=self.wandb_run.project,
                        wandb_entity=self.wandb_run.entity, wandb_group=self.wandb_run.group,
                        wandb_config=self.wandb_run.config.as_dict())
        with open(os.path.join(folder_path, "BOOK_KEEPING_VARS.json"), "w") as f:
            json.dump(book, f, indent=4)
        print(f"Checkpoint {cumulative_timesteps} saved!\n")

    def _latest_checkpoint(self):
        base = self.checkpoints_save_folder
        if base is None:
            return None
        if self.add_unix_timestamp:
            stem = base[:base.rfind("-")]
            parent = os.path.dirname(stem)
            if not os.path.exists(parent):
                return None
            runs = []
            for name in os.listdir(parent):
                full = os.path.join(parent, name)
                stamp = name[name.rfind("-") + 1:]
                if os.path.isdir(full) and full.startswith(stem) and "-" in name and stamp.isdigit():
                    runs.append((int(stamp), full))
            if not runs:
                return None
            base = max(runs)[1]
        elif not os.path.exists(base):
            return None
        steps = [int(name) for name in os.listdir(base) if name.isdigit() and os.path.isdir(os.path.join(base, name))]
        return os.path.join(base, str(max(steps))) if steps else None

    def load(self, folder_path, load_wandb, new_policy_lr=None, new_critic_lr=None):
        if folder_path == "latest":
            folder_path = self._latest_checkpoint()
            if folder_path is None:
                return
            print(f"Auto-load path: {folder_path}")
        assert os.path.exists(folder_path), f"UNABLE TO LOCATE FOLDER {folder_path}"
        print(f"Loading from checkpoint at {folder_path}")
        self.ppo_learner.load_from(folder_path)
        wandb_loaded = False
        with open(os.path.join(folder_path, "BOOK_KEEPING_VARS.json"), "r") as f:
            book = dict(json.load(f))
        self.agent.cumulative_timesteps = book["cumulative_timesteps"]
        self.agent.average_reward = book["policy_average_reward"]
        self.ppo_learner.cumulative_model_updates = book["cumulative_model_updates"]
        self.return_stats.from_json(book["reward_running_stats"])
        if self.agent.standardize_obs and "obs_running_stats" in book:
            self.agent.obs_stats = WelfordRunningStat(1)
            self.agent.obs_stats.from_json(book["obs_running_stats"])
        if self.critic_observations and self.agent.standardize_obs:
            if "critic_obs_running_stats" in book:
                self.agent.critic_obs_stats = WelfordRunningStat(1)
                self.agent.critic_obs_stats.from_json(book["critic_obs_running_stats"])
            else:
                warnings.warn("the checkpoint has no 'critic_obs_running_stats' (it was written without critic_observations): the critic's "
                              "observation statistics start fresh", RuntimeWarning, stacklevel=2)
        normalize_value = getattr(self, "normalize_value", False)
        if "value_norm_running_stats" in book:
            if not normalize_value:
                raise ValueError("the checkpoint was written with ppo_normalize_value=True (its critic puts out normalised values): "
                                 "load it into a Learner with ppo_normalize_value=True")
            self.ppo_learner.load_value_norm_state(book["value_norm_running_stats"])
            self._value_norm_host = None
        elif normalize_value:
            warnings.warn("the checkpoint has no 'value_norm_running_stats' (it was written without ppo_normalize_value): the value "
                          "statistic starts fresh, and the loaded critic's outputs are read as normalised values", RuntimeWarning, stacklevel=2)
        self.epoch = book["epoch"]
        if new_policy_lr is not None or new_critic_lr is not None:
            self.update_learning_rate(new_policy_lr, new_critic_lr)
        if "wandb_run_id" in book and load_wandb and wandb is not None:
            self.wandb_run = wandb.init(settings=wandb.Settings(start_method="spawn"), entity=book["wandb_entity"],
                                        project=book["wandb_project"], group=book["wandb_group"], id=book["wandb_run_id"],
                                        config=book["wandb_config"], resume="allow", reinit=True)
            wandb_loaded = True
        print("Checkpoint loaded!")
        return wandb_loaded

    def cleanup(self):
        if self.wandb_run is not None:
            self.wandb_run.finish()
        if type(self.agent) in (BatchedAgentManager, VectorAgentManager):
            self.agent.cleanup()
        self.experience_buffer.clear()
