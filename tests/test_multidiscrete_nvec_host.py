"""CPU checks of the general multi-discrete head (any nvec): MultiDiscreteRolv(bins) against per-head float64 Categoricals, the
argument checks of rlppo_ppo_minibatch_nvec's md_nvec / md_heads before any launch (placeholder pointers, no GPU), the Python
ValueErrors, and the signatures that keep action_mask last."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import multidiscrete_nvec_yardstick as Y

BIN_SETS = [(2, 7, 3, 11, 2), (1, 4), (33, 2, 31)]


@pytest.mark.parametrize("bins", BIN_SETS, ids=str)
def test_rolv_matches_per_head_float64_categoricals(bins):
    from rlgym_ppo_amd.util.torch_functions import MultiDiscreteRolv
    torch.manual_seed(3)
    n, H, B, S = 257, len(bins), max(bins), sum(bins)
    logits = torch.randn(n, S) * 2.0
    dist = MultiDiscreteRolv(list(bins))
    dist.make_distribution(logits)
    acts = torch.stack([torch.randint(0, b, (n,)) for b in bins], dim=1)
    want_lp, want_ent = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for h, part in enumerate(torch.split(logits.double(), list(bins), dim=-1)):
        c = torch.distributions.Categorical(logits=part)
        want_lp += c.log_prob(acts[:, h])
        want_ent += c.entropy()
    # float32 logits, as the policy hands them over: a float32 log_softmax of b values carries up to ~4 u (max|z| + log b) of
    # absolute rounding (u = 2^-24: the subtraction of the maximum, the sum, the logarithm, the final subtraction), whatever the size
    # of the result -- so the bound of this leg is absolute and summed over the heads
    lp, ent = dist.log_prob(acts).double(), dist.entropy().double()
    assert lp.shape == (n,) and ent.shape == (n,) and lp.dtype == torch.float64
    bound = sum(4 * 2.0 ** -24 * (part.abs().max(-1).values.double() + np.log(b)) for part, b in zip(torch.split(logits, list(bins), dim=-1), bins))
    assert ((lp - want_lp).abs() <= bound).all() and ((ent - want_ent).abs() <= bound).all()
    # float64 logits: the construction itself, to 1e-6 relative
    dist.make_distribution(logits.double())
    lp, ent = dist.log_prob(acts), dist.entropy()
    assert lp.dtype == torch.float64 and lp.shape == (n,) and ent.shape == (n,)
    assert ((lp - want_lp).abs() <= 1e-6 * want_lp.abs()).all()
    assert ((ent - want_ent).abs() <= 1e-6 * want_ent.abs()).all()
    dist.make_distribution(logits)
    # sample() under a seed == argmax(p / q) with the (n H, B) exponential draw of the same seed, same generator state afterwards
    torch.manual_seed(11)
    got = dist.sample()
    state = torch.get_rng_state()
    torch.manual_seed(11)
    q = torch.empty(n * H, B).exponential_(1)
    assert torch.equal(state, torch.get_rng_state())
    p = torch.softmax(Y.padded_logits(logits, bins), dim=-1).reshape(n * H, B)
    assert got.shape == (n, H) and torch.equal(got, torch.argmax(p / q, dim=-1).reshape(n, H))
    assert (got < torch.as_tensor(bins)).all()


def test_rolv_reference_bins_are_the_reference_layout():
    """The reference's bins through the general construction: [n, 8, 3] with -inf in the third slot of the 2-way heads."""
    from rlgym_ppo_amd.util.torch_functions import MultiDiscreteRolv
    torch.manual_seed(0)
    logits = torch.randn(5, 21)
    dist = MultiDiscreteRolv(list(Y.REFERENCE_BINS))
    dist.make_distribution(logits)
    want = torch.cat([logits[:, :15].reshape(5, 5, 3), torch.nn.functional.pad(logits[:, 15:].reshape(5, 3, 2), (0, 1), value=float("-inf"))], 1)
    assert torch.equal(dist.distribution.logits, want - want.logsumexp(-1, keepdim=True))


SLOT_BEYOND = 99   # every call below carries it: the slot check is the LAST argument check of rlppo_ppo_minibatch, behind the head's


def _call(head, n_out, act_dim, nvec, heads=None):
    """rlppo_ppo_minibatch_nvec with placeholder pointers and a slot that does not exist.  No such call can reach a launch: one whose
    head arguments are accepted comes back with the slot's error ("passed"), any other with the head's."""
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    pol, val = N.dims_array([107, 256, 256, 256, n_out]), N.dims_array([107, 256, 256, 256, 1])
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim, a.slot, a.precision = head, 4, 4, act_dim, SLOT_BEYOND, N.PRECISION_FP32
    a.pol_dims = ctypes.cast(pol, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(val, ctypes.POINTER(ctypes.c_int32))
    fake = iter(range(0x10000, 0x1000000, 0x1000))  # distinct, never dereferenced
    for f in ("pol_packed", "val_packed", "pol_grad", "val_grad", "states", "actions", "old_logp", "targets", "advantages", "idx",
              "stats", "workspace"):
        setattr(a, f, next(fake))
    keep = None if nvec is None else Y.nvec_array(nvec)
    n_heads = 0 if nvec is None else (len(nvec) if heads is None else heads)
    a.ld_states, a.n_rows, a.mb = 112, 5000, 1500
    a.clip_range, a.ent_coef, a.mb_ratio, a.var_m, a.var_b = 0.2, 0.005, 1.0, 1.0, 0.0
    a.ws_bytes = L.rlppo_minibatch_workspace_bytes_for(pol, 4, val, 4, a.mb, N.PRECISION_FP32)
    assert a.ws_bytes > 0
    rc, msg = L.rlppo_ppo_minibatch_nvec(None, ctypes.byref(a), keep, n_heads), L.rlppo_last_error().decode()
    assert rc == 1001, (rc, msg)
    if nvec is None:   # NULL is exactly the plain entry point
        rc0, msg0 = L.rlppo_ppo_minibatch(None, ctypes.byref(a)), L.rlppo_last_error().decode()
        assert (rc0, msg0) == (rc, msg)
    return ("passed" if f"slot {SLOT_BEYOND}" in msg else "refused"), msg


def test_ppo_minibatch_checks_md_nvec_before_any_launch():
    """Following tests/test_abi_and_layout.py::test_ppo_minibatch_rejects_bad_arguments_before_any_launch: placeholder pointers,
    no GPU.  Every bad nvec is error 1001 with a message naming the argument and the limit; a NULL nvec with 21 outputs passes
    the head check as before."""
    from rlgym_ppo_amd import _native as N
    MD, bins = N.HEAD_MULTIDISCRETE, (2, 7, 3, 11, 2)
    call = _call
    verdict, msg = call(MD, 26, 5, bins)                       # sum(nvec) = 25, the policy has 26 outputs
    assert verdict == "refused" and "md_nvec" in msg and "25" in msg and "26" in msg, msg
    verdict, msg = call(MD, 25, 4, bins)                       # act_dim != md_heads
    assert verdict == "refused" and "act_dim=4" in msg and "md_heads=5" in msg, msg
    verdict, msg = call(MD, 130, 65, (2,) * 65)                # H = 65
    assert verdict == "refused" and "md_heads" in msg and "65 heads" in msg and "RLPPO_MD_MAX_HEADS" in msg, msg
    verdict, msg = call(MD, 25, 5, bins, heads=0)              # H = 0
    assert verdict == "refused" and "RLPPO_MD_MAX_HEADS" in msg, msg
    verdict, msg = call(MD, 23, 5, (2, 7, 3, 0, 11))           # a bin of 0
    assert verdict == "refused" and "md_nvec" in msg and "nvec[3]=0" in msg and "RLPPO_MD_MAX_BINS" in msg, msg
    verdict, msg = call(MD, 79, 3, (2, 65, 12))                # a bin of 65
    assert verdict == "refused" and "md_nvec" in msg and "nvec[1]=65" in msg and "RLPPO_MD_MAX_BINS" in msg, msg
    verdict, msg = call(MD, 513, 9, (64,) * 8 + (1,))          # S = 513 > 512
    assert verdict == "refused" and "md_nvec" in msg and "RLPPO_MD_MAX_LOGITS" in msg and "513" in msg, msg
    verdict, msg = call(N.HEAD_DISCRETE, 90, 1, bins)          # md_nvec with the discrete head
    assert verdict == "refused" and "md_nvec" in msg and "discrete" in msg, msg
    verdict, msg = call(N.HEAD_GAUSSIAN, 16, 8, bins)
    assert verdict == "refused" and "md_nvec" in msg and "Gaussian" in msg, msg
    verdict, msg = call(MD, 25, 5, None)                       # NULL nvec, 25 outputs: refused as before
    assert verdict == "refused" and "21 outputs" in msg, msg
    # what the head checks accept
    assert call(MD, 21, 8, None)[0] == "passed"                # NULL nvec, 21 outputs: as before
    assert call(MD, 25, 5, bins)[0] == "passed"
    assert call(MD, 21, 8, Y.REFERENCE_BINS)[0] == "passed"
    assert call(MD, 512, 8, (64,) * 8)[0] == "passed"          # S at its cap
    assert call(MD, 128, 64, (2,) * 64)[0] == "passed"         # H at its cap
    assert call(MD, 5, 2, (1, 4))[0] == "passed"               # a head of one bin


def test_header_names_the_limits_and_the_entry_point():
    from rlgym_ppo_amd import _native as N
    header = open(N.HERE + "/../include/rlppo.h").read()
    for name, value in (("RLPPO_MD_MAX_HEADS", N.MD_MAX_HEADS), ("RLPPO_MD_MAX_BINS", N.MD_MAX_BINS), ("RLPPO_MD_MAX_LOGITS", N.MD_MAX_LOGITS)):
        assert f"#define {name} {value}\n" in header
    assert (N.MD_MAX_HEADS, N.MD_MAX_BINS, N.MD_MAX_LOGITS) == (64, 64, 512)
    res, args = N.SIGNATURES["rlppo_multidiscrete_act_nvec"]
    plain = N.SIGNATURES["rlppo_multidiscrete_act"]
    assert res == plain[0] and args == plain[1] + [ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
    res, args = N.SIGNATURES["rlppo_ppo_minibatch_nvec"]
    plain = N.SIGNATURES["rlppo_ppo_minibatch"]
    assert res == plain[0] and args == plain[1] + [ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
    assert "int rlppo_ppo_minibatch_nvec(" in header and "int rlppo_multidiscrete_act_nvec(" in header
    assert [f[0] for f in N.MinibatchArgs._fields_][-2:] == ["action_mask", "mask_words"]   # the struct is as it was: the entry points are additions
    assert N.lib().rlppo_dbg_counter(6) >= 0


def test_act_nvec_checks_its_arguments_before_any_launch():
    """rlppo_multidiscrete_act_nvec with placeholder pointers: a mask is refused with the existing text, nvec against the limits and
    against the output width."""
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    fake = [ctypes.c_void_p(0x100000 + 0x10000 * k) for k in range(6)]

    def call(n_out, nvec, heads=None, opts=None):
        dims = N.dims_array([20, 64, 64, n_out])
        keep = Y.nvec_array(nvec)
        rc = L.rlppo_multidiscrete_act_nvec(None, dims, 3, fake[0], fake[1], 32, 10, fake[2], fake[3], fake[4], fake[5], 0, opts,
                                            keep, len(nvec) if heads is None else heads)
        return rc, L.rlppo_last_error().decode()

    rc, msg = call(26, (2, 7, 3, 11, 2))
    assert rc == 1001 and "26" in msg and "25" in msg, (rc, msg)
    rc, msg = call(130, (2,) * 65)
    assert rc == 1001 and "RLPPO_MD_MAX_HEADS" in msg, (rc, msg)
    rc, msg = call(66, (65, 1))
    assert rc == 1001 and "RLPPO_MD_MAX_BINS" in msg, (rc, msg)
    rc, msg = call(513, (64,) * 8 + (1,))
    assert rc == 1001 and "RLPPO_MD_MAX_LOGITS" in msg, (rc, msg)
    o = N.ActOpts()
    o.action_mask, o.mask_words = 0x200000, 1
    rc, msg = call(25, (2, 7, 3, 11, 2), opts=ctypes.byref(o))
    rc0 = L.rlppo_multidiscrete_act(None, N.dims_array([20, 64, 64, 21]), 3, fake[0], fake[1], 32, 10, fake[2], fake[3], fake[4], fake[5], 0,
                                    ctypes.byref(o))
    msg0 = L.rlppo_last_error().decode()
    assert rc == 1001 == rc0 and "action_mask" in msg and "multi-discrete" in msg, (rc, msg)
    assert msg.replace("rlppo_multidiscrete_act_nvec", "rlppo_multidiscrete_act") == msg0   # the existing text


def test_python_value_errors():
    from rlgym_ppo_amd.ppo import PPOLearner
    from rlgym_ppo_amd.ppo.multi_discrete_policy import MultiDiscreteFF, check_bins
    args = ((64, 64), (64, 64), (0.1, 1.0), 64, 1, 3e-4, 3e-4, 0.2, 0.005, 64, "cuda:0")
    # (the checks precede everything that needs a GPU).  PPOLearner takes the bins as act_space_size: with another policy type a
    # sequence there is refused
    with pytest.raises(ValueError, match="policy_type 0"):
        PPOLearner(20, (2, 7, 3, 11, 2), 0, *args)
    with pytest.raises(ValueError, match="policy_type 2"):
        PPOLearner(20, [2, 7, 3, 11, 2], 2, *args)
    for bad in ((), (2,) * 65, (0, 3), (65,), (64,) * 8 + (1,), (2.5, 3)):
        with pytest.raises(ValueError, match="bins"):
            check_bins(bad)
        with pytest.raises(ValueError, match="bins"):
            MultiDiscreteFF(20, (64, 64), "cuda:0", bins=bad)
        with pytest.raises(ValueError, match="bins"):
            PPOLearner(20, bad, 1, *args)
    for bad in ("ab", 7):
        with pytest.raises(ValueError, match="bins"):
            check_bins(bad)
    assert check_bins(np.array([2, 7, 3])) == [2, 7, 3] and check_bins((64,) * 8) == [64] * 8 and check_bins([2] * 64) == [2] * 64


class _Agent:
    """Stand-in for the collection manager: an environment of 8 action components, type code `code`."""
    def __init__(self, *a, **k):
        self.code = _Agent.code

    def init_processes(self, **k):
        return (20,), 8, self.code

    def cleanup(self):
        pass


@pytest.mark.parametrize("code,match", [(1, "5 entries.*8 components"), (0, "type 0"), (2, "type 2")])
def test_learner_refuses_bins_that_do_not_fit_the_action_space(monkeypatch, tmp_path, code, match):
    """Learner(multi_discrete_bins=...): len(bins) != the action space's size, or another action space type, is a ValueError --
    raised before the PPOLearner (and with it the GPU) is touched."""
    import torch
    from rlgym_ppo_amd import learner as LM
    _Agent.code = code
    monkeypatch.setattr(LM, "BatchedAgentManager", _Agent)
    monkeypatch.setattr(LM, "ExperienceBuffer", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    with pytest.raises(ValueError, match=match):
        LM.Learner(lambda: None, device="cuda:0", multi_discrete_bins=(2, 7, 3, 11, 2), checkpoints_save_folder=str(tmp_path / "c"),
                   add_unix_timestamp=False, checkpoint_load_folder=None)


def test_signatures_keep_action_mask_last_and_bins_optional():
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd.ppo import PPOLearner
    from rlgym_ppo_amd.ppo.multi_discrete_policy import MultiDiscreteFF
    for name in ("get_action", "act_padded", "get_output", "get_backprop_data"):
        ps = list(inspect.signature(getattr(MultiDiscreteFF, name)).parameters.values())
        assert ps[-1].name == "action_mask" and ps[-1].default is None, name
    with pytest.raises(ValueError, match="multi-discrete"):
        MultiDiscreteFF.get_output(object.__new__(MultiDiscreteFF), None, action_mask=np.ones((1, 3)))
    ps = inspect.signature(MultiDiscreteFF.__init__).parameters
    assert list(ps) == ["self", "input_shape", "layer_sizes", "device", "bins"] and ps["bins"].default is None
    ps = inspect.signature(PPOLearner.__init__).parameters   # (its parameter list stays the reference's + the four options)
    assert "multi_discrete_bins" not in ps and list(ps)[2] == "act_space_size"
    ps = inspect.signature(Learner.__init__).parameters
    assert "multi_discrete_bins" in ps and ps["multi_discrete_bins"].default is None
