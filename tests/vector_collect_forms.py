"""The matrix that holds every form of VectorAgentManager's collect to every other (tests/test_gpu_vector_collect_forms.py) and a
tree to its parent (tools/vector_collect_equivalence.py).  It reaches the manager through `collect_timesteps`, its public attributes
and `_next_rows` only, so the same file drives any checkout.

A form is (interface, fused_step): the environment behind the host (numpy) or the device interface, and -- for DiscreteFF -- the
one-launch `policy.step` or `stage_obs` + `act_padded`.  A case is (head, n_agents, feature, standardize); every form of a case sees
the same interaction sequence, so every output of its three collects (T = 1, then 9, then a ragged request with T = 5: 15 steps that
cross the statistics cadence twice) must be the same bytes.  32 x 32 networks from one seed per head; observations of width 13."""
import hashlib

import numpy as np
import torch

import critic_obs_env as CE
import device_vector_env as E

DEV = "cuda:0"
OBS, HID, BINS = CE.OBS, (32, 32), (2, 7, 3)
WIDTH = {"discrete": CE.N_ACTIONS, "multidiscrete": sum(BINS)}   # mask entries per agent
N_AGENTS = (1, 3, 16)
FEATURES = {"discrete": ("none", "masks", "critic", "bootstrap", "masks+critic"), "gaussian": ("none", "critic", "bootstrap"),
            "multidiscrete": ("none", "masks", "critic", "bootstrap", "masks+critic")}
EXPERIENCE = ("states", "actions", "log_probs", "rewards", "next_states", "dones", "truncated")


def requests(na):
    """-> the three request sizes: T = 1 (the flush step is the first step), T = 9, T = 5 from a request that is no multiple of na."""
    return (na, 9 * na, 5 * na - na // 2)


def cases():
    out = []
    for head, features in FEATURES.items():
        for na in N_AGENTS:
            for feature in features:
                for standardize in ((True, False, "per_feature") if head == "discrete" else (True,)):
                    out.append(dict(head=head, n_agents=na, feature=feature, standardize=standardize))
    return out


def case_id(case):
    return "-".join(str(case[k]) for k in ("head", "n_agents", "feature", "standardize"))


def forms(head):
    fused = (True, False) if head == "discrete" else (None,)
    return [(side, f) for side in ("host", "device") for f in fused]


class MaskedCriticEnv(CE.CriticVectorEnv):
    """CriticVectorEnv with action_masks(): a third of the entries invalid, moving with the step counter (no head is left empty)."""
    width = CE.N_ACTIONS

    def action_masks(self):
        return (np.arange(self.width)[None, :] + self.t + np.arange(self.n_agents)[:, None]) % 3 != 0


def make_policy(head):
    from rlgym_ppo_amd.ppo import DiagGaussianPolicy, DiscreteFF, MultiDiscreteFF
    torch.manual_seed(11)
    if head == "gaussian":
        return DiagGaussianPolicy(OBS, 3, HID, DEV, log_std_init=0.25)
    if head == "multidiscrete":
        return MultiDiscreteFF(OBS, HID, DEV, bins=BINS)
    return DiscreteFF(OBS, CE.N_ACTIONS, HID, DEV)


def make_env(case, side):
    head, na, feature = case["head"], case["n_agents"], case["feature"]
    if "critic" in feature:
        env = (MaskedCriticEnv if "masks" in feature else CE.CriticVectorEnv)(n_agents=na, alias=False)
        env.width = WIDTH.get(head)
        return CE.CriticDeviceTwin(env) if side == "device" else env
    return E.IntegerEnv(n_agents=na, obs_dim=OBS, n_actions=WIDTH.get(head, 3), device=torch.device(DEV) if side == "device" else None,
                        masks=feature == "masks", final_obs=feature == "bootstrap")


def make_manager(case, side, fused):
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    from rlgym_ppo_amd.ppo import ValueEstimator
    pol = make_policy(case["head"])
    if fused is not None:
        pol.fused_step = fused
    mgr = VectorAgentManager(pol, seed=5, standardize_obs=bool(case["standardize"]))
    mgr.per_feature_obs_standardization = case["standardize"] == "per_feature"
    mgr.bootstrap_truncated = case["feature"] == "bootstrap"
    if "critic" in case["feature"]:
        torch.manual_seed(12)
        mgr.critic_observations, mgr.value_net = True, ValueEstimator(CE.CRITIC_OBS, HID, DEV)
    mgr.init_processes(0, lambda: make_env(case, side))
    return mgr


def _bytes(x):
    if x is None:
        return b"none"
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x)
    return repr((x.dtype.str, x.shape)).encode() + x.tobytes()


def outputs(mgr, exp):
    """-> ({name: bytes} of everything every form of a case must agree on, the bootstrap outputs in this form's own shape)."""
    out = {name: _bytes(t) for name, t in zip(EXPERIENCE, exp)}
    assert exp[0].data_ptr() == mgr.value_input_rows.data_ptr()
    out["value_input_rows"], out["_next_rows"] = _bytes(mgr.value_input_rows), _bytes(mgr._next_rows)
    out["action_mask_words"] = _bytes(None if mgr.action_mask_rows is None else mgr.action_mask_rows.words)
    out["critic_value_input_rows"] = _bytes(mgr.critic_value_input_rows)
    for name, st in (("obs_stats", mgr.obs_stats), ("critic_obs_stats", mgr.critic_obs_stats)):
        out[name] = b"none" if st is None else _bytes(np.int64(st.count)) + _bytes(st.running_mean) + _bytes(st.running_variance)
    out["average_reward"] = _bytes(None if mgr.average_reward is None else np.float64(mgr.average_reward))
    out["cumulative_timesteps"] = _bytes(np.int64(mgr.cumulative_timesteps))
    out["rng_state"] = _bytes(torch.get_rng_state())
    boot = None
    if mgr.bootstrap_truncated:
        if mgr.bootstrap_dense:
            boot = dict(dense=mgr.bootstrap_rows.detach().cpu().numpy())
        else:
            boot = dict(steps=np.asarray(mgr.bootstrap_steps), rows=mgr.bootstrap_rows.detach().cpu().numpy())
    return out, boot


def run_form(case, side, fused, flip=False):
    """Three consecutive collects on one manager -> [(outputs, bootstrap)] per collect.  flip: policy.fused_step is turned over between
    the second and the third collect."""
    mgr = make_manager(case, side, fused)
    got = []
    try:
        for i, n in enumerate(requests(case["n_agents"])):
            if flip and i == 2:
                mgr.policy.fused_step = not fused
            torch.manual_seed(100 + i)
            exp, _, n_col, _ = mgr.collect_timesteps(n)
            assert n_col == exp[0].shape[0] == -(-n // case["n_agents"]) * case["n_agents"]
            got.append(outputs(mgr, exp))
    finally:
        mgr.cleanup()
    return got


def check_bootstrap(host, device):
    """The host forms' sparse answer against the device form's dense rows at those steps."""
    assert np.array_equal(host["rows"].view(np.uint8), device["dense"][host["steps"]].view(np.uint8))


def digest(results):
    """{form name: run_form's answer} -> one sha256 over every output of every form and collect, in a fixed order."""
    h = hashlib.sha256()
    for form in sorted(results):
        for out, boot in results[form]:
            for name in sorted(out):
                h.update(name.encode() + hashlib.sha256(out[name]).digest())
            for name in sorted(boot or {}):
                h.update(name.encode() + hashlib.sha256(_bytes(boot[name])).digest())
    return h.hexdigest()


def form_name(side, fused):
    return side + {None: "", True: "-step", False: "-chain"}[fused]


FLIP_CASE = dict(head="discrete", n_agents=3, feature="masks+critic", standardize=True)
