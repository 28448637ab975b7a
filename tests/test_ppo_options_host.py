"""CPU checks of the options beyond the reference (PPOLearner / Learner keyword arguments, their defaults, the report printer):
no GPU, no compute call."""
import inspect

import numpy as np


def test_ppo_learner_options_and_defaults():
    from rlgym_ppo_amd.ppo import PPOLearner
    params = inspect.signature(PPOLearner.__init__).parameters
    names = list(params)
    assert names[1:15] == ["obs_space_size", "act_space_size", "policy_type", "policy_layer_sizes", "critic_layer_sizes",
                           "continuous_var_range", "batch_size", "n_epochs", "policy_lr", "critic_lr", "clip_range", "ent_coef",
                           "mini_batch_size", "device"]                              # the reference's 14 positionals, unchanged
    assert names[15:] == ["normalize_advantages", "value_clip_range", "target_kl", "max_grad_norm"]
    defaults = {k: params[k].default for k in names[15:]}
    assert defaults == {"normalize_advantages": False, "value_clip_range": None, "target_kl": None, "max_grad_norm": 0.5}


def test_learner_options_and_defaults():
    from rlgym_ppo_amd import Learner
    params = inspect.signature(Learner.__init__).parameters
    names = list(params)
    i = names.index("per_feature_obs_standardization")
    assert names[i + 1:] == ["ppo_normalize_advantages", "ppo_value_clip_range", "ppo_target_kl", "ppo_max_grad_norm"]
    assert [params[k].default for k in names[i + 1:]] == [False, None, None, 0.5]


def _report():
    keys = ["Policy Reward", "Policy Entropy", "Value Function Loss", "Mean KL Divergence", "SB3 Clip Fraction", "Policy Update Magnitude",
            "Value Function Update Magnitude", "Collected Steps per Second", "Overall Steps per Second", "Timestep Collection Time",
            "Timestep Consumption Time", "PPO Batch Consumption Time", "Total Iteration Time", "Cumulative Model Updates",
            "Cumulative Timesteps", "Timesteps Collected"]
    rep = {k: 0.25 for k in keys}
    rep["Cumulative Model Updates"], rep["Cumulative Timesteps"], rep["Timesteps Collected"] = 12, 3000, 1000
    rep["Policy Reward"] = np.nan
    return rep


def test_reporting_default_report_has_no_option_keys(capsys):
    from rlgym_ppo_amd.util import reporting
    reporting.report_metrics(_report(), None)
    out = capsys.readouterr().out
    assert "Mean KL Divergence" in out and "Cumulative Model Updates: 12" in out
    assert "PPO Optimizer Steps" not in out and "KL Early Stopped" not in out


def test_reporting_prints_the_target_kl_keys_when_present(capsys):
    from rlgym_ppo_amd.util import reporting
    rep = _report()
    rep["PPO Optimizer Steps"] = 7
    rep["KL Early Stopped"] = 1.0
    reporting.report_metrics(rep, None)
    out = capsys.readouterr().out
    assert "PPO Optimizer Steps: 7" in out and "KL Early Stopped: 1.00000" in out
    assert out.index("Timesteps Collected") < out.index("PPO Optimizer Steps")
