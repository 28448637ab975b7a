"""Invalid-action masking of the multi-discrete head, the parts that need no GPU: the per-head check of util/action_mask.py, the
argument checks of rlppo_ppo_minibatch_nvec / rlppo_multidiscrete_act_nvec_masked with a mask (placeholder pointers: the checks run before
any HIP call), the yardstick's masked sampling against a seeded CPU Categorical, and the refusals that stay."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nets
import masked_multidiscrete_yardstick as M
import multidiscrete_nvec_yardstick as Y
import ppo_yardstick as PY

BINS = (2, 7, 3, 11, 2)


def test_per_head_check_names_row_and_head():
    from rlgym_ppo_amd.util import action_mask as AM
    S = sum(BINS)
    m = np.ones((9, S), bool)
    m[4, 2:9] = False            # head 1 (bins 2 .. 8) of row 4 has no valid bin
    for form in (m, torch.from_numpy(m), m.astype(np.float32)):
        with pytest.raises(ValueError, match=r"row 4, head 1"):
            AM.pack(form, S, "cpu", heads=BINS)
    with pytest.raises(ValueError, match=r"row 4, head 1"):
        AM.check_heads(m, BINS)
    assert AM.pack(m, S, "cpu") is not None             # the per-row rule alone accepts it: the row has valid entries
    m[4, 5] = True                                       # exactly one valid bin: fine
    m[7, :] = False
    m[7, [1, 8, 9, 22, 24]] = True                       # every head exactly one, the last bins among them
    AM.check_heads(m, BINS)
    words = AM.pack(m, S, "cpu", heads=BINS)
    assert tuple(words.shape) == (9, 1) and np.array_equal(AM.unpack(words, S).numpy(), m)
    with pytest.raises(ValueError, match="shape"):
        AM.check_heads(np.ones((3, S + 1), bool), BINS)
    wide = (64,) * 8                                     # a head in words 14 .. 15 of 16
    mw = np.ones((3, 512), bool)
    mw[2, 448:512] = False
    with pytest.raises(ValueError, match=r"row 2, head 7"):
        AM.pack(mw, 512, "cpu", heads=wide)


def _minibatch_call(bins, n_out, mask_words, nvec=True, head=None):
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    pol, val = N.dims_array([107, 256, 256, 256, n_out]), N.dims_array([107, 256, 256, 256, 1])
    a = N.MinibatchArgs()
    a.head = N.HEAD_MULTIDISCRETE if head is None else head
    a.pol_layers, a.val_layers, a.act_dim, a.slot, a.precision = 4, 4, len(bins), 0, N.PRECISION_FP32
    a.pol_dims = ctypes.cast(pol, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(val, ctypes.POINTER(ctypes.c_int32))
    fake = iter(range(0x10000, 0x1000000, 0x1000))  # distinct, never dereferenced
    for f in ("pol_packed", "val_packed", "pol_grad", "val_grad", "states", "actions", "old_logp", "targets", "advantages", "idx", "stats",
              "workspace", "action_mask"):
        setattr(a, f, next(fake))
    a.mask_words = mask_words
    a.ld_states, a.n_rows, a.mb = 112, 5000, 1500
    a.clip_range, a.ent_coef, a.mb_ratio, a.var_m, a.var_b = 0.2, 0.005, 1.0, 1.0, 0.0
    a.ws_bytes = L.rlppo_minibatch_workspace_bytes_for(pol, 4, val, 4, a.mb, N.PRECISION_FP32)
    keep = Y.nvec_array(bins)
    rc = L.rlppo_ppo_minibatch_nvec(None, ctypes.byref(a), keep if nvec else None, len(bins))
    return rc, L.rlppo_last_error().decode()


def test_minibatch_nvec_checks_mask_words_before_any_launch():
    """md_nvec given and a wrong mask_words: 1001, naming the field and the needed count (not the refusal of the fixed-bin form)."""
    for bins, bad, need in ((BINS, (0, 2), "1"), ((30, 64, 5), (1, 3, 5), "4"), ((64,) * 8, (15, 17), "16"), (Y.REFERENCE_BINS, (2,), "1")):
        for w in bad:
            rc, msg = _minibatch_call(bins, sum(bins), w)
            assert rc == 1001 and "mask_words" in msg and need in msg and "option of the discrete head" not in msg, (bins, w, rc, msg)
    # the fixed-bin form (md_nvec NULL) keeps refusing a mask, also with the right word count
    rc, msg = _minibatch_call(Y.REFERENCE_BINS, 21, 1, nvec=False)
    assert rc == 1001 and "action_mask" in msg and "multi-discrete" in msg, (rc, msg)


def test_act_nvec_masked_checks_mask_words_and_a_mask_in_the_options_stays_refused():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    fake = [ctypes.c_void_p(0x100000 + 0x10000 * k) for k in range(6)]
    words = ctypes.c_void_p(0x200000)

    def masked(bins, mask, mask_words, opts=None):
        rc = L.rlppo_multidiscrete_act_nvec_masked(None, N.dims_array([20, 64, 64, sum(bins)]), 3, fake[0], fake[1], 32, 10, fake[2], fake[3],
                                                   fake[4], fake[5], 0, opts, Y.nvec_array(bins), len(bins), mask, mask_words)
        return rc, L.rlppo_last_error().decode()

    for bins, bad, need in ((BINS, 2, "1"), ((30, 64, 5), 3, "4"), ((64,) * 8, 1, "16")):
        rc, msg = masked(bins, words, bad)
        assert rc == 1001 and "mask_words" in msg and need in msg, (bins, rc, msg)
    rc, msg = masked(BINS, None, 1)
    assert rc == 1001 and "action_mask is NULL" in msg, (rc, msg)
    rc, msg = masked((2,) * 65, words, 5)
    assert rc == 1001 and "RLPPO_MD_MAX_HEADS" in msg, (rc, msg)
    o = N.ActOpts()
    o.action_mask, o.mask_words = 0x200000, 1
    rc, msg = masked(BINS, words, 1, ctypes.byref(o))            # the mask is an argument, never an option
    assert rc == 1001 and "action_mask" in msg and "multi-discrete" in msg, (rc, msg)
    rc = L.rlppo_multidiscrete_act_nvec(None, N.dims_array([20, 64, 64, 25]), 3, fake[0], fake[1], 32, 10, fake[2], fake[3], fake[4], fake[5], 0,
                                        ctypes.byref(o), Y.nvec_array(BINS), 5)
    msg = L.rlppo_last_error().decode()
    assert rc == 1001 and "action_mask" in msg and "multi-discrete" in msg, (rc, msg)
    rc = L.rlppo_multidiscrete_act(None, N.dims_array([20, 64, 64, 21]), 3, fake[0], fake[1], 32, 10, fake[2], fake[3], fake[4], fake[5], 0,
                                   ctypes.byref(o))
    msg = L.rlppo_last_error().decode()
    assert rc == 1001 and "action_mask" in msg and "multi-discrete" in msg, (rc, msg)


def test_yardstick_masked_sampling_is_the_seeded_cpu_categorical():
    """masked_sample64 on float32 CPU logits == Categorical(logits=masked_padded).sample() under the same seed (whose multinomial
    draws torch.empty(n H, B).exponential_(1): nets.draw_exp_noise), except at near-ties; invalid bins are never drawn."""
    n, S, H = 300, sum(BINS), len(BINS)
    rs = np.random.RandomState(8)
    z = torch.from_numpy((rs.randn(n, S) * 2).astype(np.float32))
    mask = M.rand_mask(rs, n, BINS)
    assert mask[0].sum() == H and mask[0, S - 1] and mask[3].all()
    torch.manual_seed(31)
    q = nets.draw_exp_noise(n * H, max(BINS))
    state = torch.get_rng_state()
    torch.manual_seed(31)
    masked = z.masked_fill(~torch.from_numpy(mask), float("-inf"))
    cpu_act = torch.distributions.Categorical(logits=Y.padded_logits(masked, BINS)).sample().numpy()
    assert torch.equal(state, torch.get_rng_state())
    act, logp, score, near = M.masked_sample64(z.numpy().astype(np.float64), BINS, q.numpy(), mask)
    assert int(near.sum()) <= 2
    v3 = M.head_valid(mask, BINS)
    assert np.take_along_axis(v3, act[..., None], -1).all() and np.take_along_axis(v3, cpu_act[..., None], -1).all()
    differ = np.argwhere(cpu_act != act)
    assert len(differ) <= 2 and all(near[r, h] for r, h in differ.tolist())
    assert (act[0] == np.asarray(BINS) - 1).all() and np.isfinite(logp).all() and logp[0] == 0.0   # one valid bin per head: log p 0
    # all-valid mask: the unmasked yardstick
    a0, l0, _, _ = Y.sample64(z.numpy().astype(np.float64), BINS, q.numpy())
    a1, l1, _, _ = M.masked_sample64(z.numpy().astype(np.float64), BINS, q.numpy(), np.ones((n, S), bool))
    assert np.array_equal(a0, a1) and np.array_equal(l0, l1)


def test_masked_chain_with_an_all_valid_mask_is_the_oracles_multidiscrete_minibatch(monkeypatch):
    """The restated chain against oracle/ppo.py on the case it can express: no bin masked."""
    from oracle import ppo
    bins = (2, 5, 3)
    pol, val, pr, rs = M.make_problem(bins, 3, 200, d=20, hidden=(32, 32))
    Y.patch_oracle(monkeypatch, bins)
    ones = np.ones_like(pr["mask"])
    logp = M.masked_logp64(Y.logits64(pol, pr["obs"]), bins, pr["acts"], ones)
    old = (logp - 0.2 * rs.randn(200)).astype(np.float32)
    want = ppo.minibatch_analytic("multidiscrete", pol, val, pr["obs"], pr["acts"], old, pr["adv"], pr["tgt"], 0.2, 0.005, 0.5, (0.1, 1.0))
    gp, gv, stats, _ = PY.masked_chain("nvec", pol, val, pr["obs"], pr["acts"], old, pr["adv"], pr["tgt"], ones, 0.5, torch.float64, bins=bins)
    import fp64_gate
    assert fp64_gate.grads_err(gp + gv, want["grad_policy"] + want["grad_value"]) < 1e-9
    for k, name in ((0, "entropy"), (1, "kl"), (2, "value_loss"), (4, "policy_loss")):
        assert abs(stats[k] - float(want[name])) <= 1e-10 * max(1.0, abs(float(want[name]))), name


def test_refusals_that_stay_and_signatures():
    import inspect
    from rlgym_ppo_amd.ppo.multi_discrete_policy import MultiDiscreteFF
    with pytest.raises(ValueError, match="multi-discrete"):
        MultiDiscreteFF.get_output(object.__new__(MultiDiscreteFF), None, action_mask=np.ones((1, 25)))
    for name in ("get_action", "act_padded", "get_output", "get_backprop_data"):
        ps = list(inspect.signature(getattr(MultiDiscreteFF, name)).parameters.values())
        assert ps[-1].name == "action_mask" and ps[-1].default is None, name
    # process-mode collection still refuses a mask for action-space types other than the discrete one, by name
    from rlgym_ppo_amd.batched_agents import batched_agent_manager as BM
    src = inspect.getsource(BM.BatchedAgentManager._configure_masking)
    assert "option of the discrete head" in src
    from rlgym_ppo_amd import _native as N
    header = open(N.HERE + "/../include/rlppo.h").read()
    assert "[nvec, masked]" in header and "int rlppo_multidiscrete_act_nvec_masked(" in header
    res, args = N.SIGNATURES["rlppo_multidiscrete_act_nvec_masked"]
    plain = N.SIGNATURES["rlppo_multidiscrete_act_nvec"]
    assert res == plain[0] and args == plain[1] + [ctypes.c_void_p, ctypes.c_int32] and N.ABI_VERSION == 8


def _manager(policy_cls, mask, **attrs):
    """A VectorAgentManager around an uninitialised policy object (CPU only) whose environment answers `mask`."""
    from rlgym_ppo_amd.batched_agents.vector_agent_manager import VectorAgentManager

    class Arena:
        device = "cpu"

    class Env:
        def action_masks(self):
            return mask

    pol = object.__new__(policy_cls)
    pol.__dict__.update(attrs, arena=Arena())
    mgr = VectorAgentManager(pol)
    mgr.env = Env()
    return mgr


def test_vector_manager_mask_shapes_for_both_heads():
    """A one-agent environment may answer a rank-1 [n_actions] mask (the discrete head's documented form, and the multi-discrete
    head's [sum(bins)]); a wrong width names both numbers; the layout is the policy's own (util.action_mask.Layout.of)."""
    from rlgym_ppo_amd.ppo.discrete_policy import DiscreteFF
    from rlgym_ppo_amd.ppo.multi_discrete_policy import MultiDiscreteFF
    from rlgym_ppo_amd.util import action_mask as AM
    m1 = np.array([1, 0, 1, 1, 0, 0, 1], bool)
    mgr = _manager(DiscreteFF, m1, n_actions=7)
    words = mgr._env_mask()
    assert tuple(words.shape) == (1, 1) and np.array_equal(AM.unpack(words, 7).numpy(), m1[None])
    assert np.array_equal(AM.unpack(_manager(DiscreteFF, np.stack([m1, ~m1]), n_actions=7)._env_mask(), 7).numpy(), np.stack([m1, ~m1]))
    with pytest.raises(ValueError, match=r"7\).*must be 9"):
        _manager(DiscreteFF, m1, n_actions=9)._env_mask()
    S = sum(BINS)
    md = dict(n_logits=S, splits=list(BINS), mask_layout=AM.Layout(S, BINS))
    row = np.ones(S, bool)
    row[3:9] = False                                   # head 1 keeps its first bin only
    mgr = _manager(MultiDiscreteFF, row, **md)
    assert np.array_equal(AM.unpack(mgr._env_mask(), S).numpy(), row[None])
    lay = AM.Layout.of(mgr.policy)
    assert lay is mgr.policy.mask_layout and lay.width == S and lay.heads == tuple(BINS) and lay.words == 1
    duck = AM.Layout.of(_manager(MultiDiscreteFF, row, n_logits=S, splits=list(BINS)).policy)   # (no mask_layout: n_logits, splits)
    assert duck.width == S and duck.heads == tuple(BINS)
    flat = AM.Layout.of(_manager(DiscreteFF, m1, n_actions=7).policy)
    assert flat.width == 7 and flat.heads is None
    with pytest.raises(ValueError, match=r"5.*must be 25"):
        _manager(MultiDiscreteFF, np.ones((12, len(BINS)), bool), **md)._env_mask()
    row[2] = False                                     # head 1 without a valid bin
    with pytest.raises(ValueError, match="row 0, head 1"):
        _manager(MultiDiscreteFF, row, **md)._env_mask()
    from rlgym_ppo_amd.ppo.continuous_policy import ContinuousPolicy
    with pytest.raises(ValueError, match="ContinuousPolicy"):
        _manager(ContinuousPolicy, m1)._env_mask()
