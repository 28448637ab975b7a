"""CPU checks of residual hidden layers (ppo.LayerSizes(..., residual=True), Learner(hidden_residual=...); include/rlppo.h, "[res]"):
the tuple, the torch module against the recurrence written out, and the refusals -- the C-level ones on a null stream with placeholder
pointers, so they come before any HIP call.  No GPU."""
import ctypes
import pickle

import pytest
import torch
import torch.nn.functional as F

from test_diag_gaussian_host import _args  # placeholder arguments of a pass


def test_layer_sizes_carry_the_flag():
    from rlgym_ppo_amd.ppo import LayerSizes
    ls = LayerSizes((32, 32), "tanh", "layer", None, True)
    back = pickle.loads(pickle.dumps(ls))
    assert ls == (32, 32) and (back, back.residual, back.norm) == (ls, True, "layer") and eval(repr(ls)).residual is True
    assert LayerSizes((8, 4)).residual is False and repr(LayerSizes((8,), "elu")) == "LayerSizes((8,), 'elu')"
    for sizes, flag, text in (((32, 32, 48, 16), True, "equal hidden widths: hidden layer 2 has 48 outputs, hidden layer 0 has 32"),
                              ((2049, 2049), True, "wider than 2048"), ((8,), "yes", "residual must be")):
        with pytest.raises(ValueError, match=text):
            LayerSizes(sizes, residual=flag)


@pytest.mark.parametrize("norm", [None, "layer"])
@pytest.mark.parametrize("act", ["relu", "tanh", "elu"])
def test_build_body_is_the_recurrence_on_the_same_weights(act, norm):
    from rlgym_ppo_amd.ppo import LayerSizes
    from rlgym_ppo_amd.ppo._mlp import activation_of, build_body, linears_of, norm_of, residual_of
    torch.manual_seed(3)
    plain = build_body(13, LayerSizes((32, 32, 32), act, norm), 6)
    torch.manual_seed(3)
    body = build_body(13, LayerSizes((32, 32, 32), act, norm, None, True), 6).double()
    sd, ref = body.state_dict(), plain.state_dict()
    assert list(sd) == list(ref) and all(torch.equal(sd[k].float(), ref[k]) for k in ref) and len(body) == len(plain)
    assert (activation_of(body), norm_of(body), residual_of(body), residual_of(plain), len(linears_of(body))) == (act, norm, True, False, 4)
    x = torch.randn(7, 13, dtype=torch.float64)
    N_ = (lambda s: F.layer_norm(s, (32,), eps=1e-5)) if norm else (lambda s: s)
    s = getattr(F, act)(body[0](x))
    for i in (2, 4):
        s = s + getattr(F, act)(body[i](N_(s)))
    assert torch.equal(body(x), body[6](N_(s)))
    one = build_body(13, LayerSizes((32,), act, norm, None, True), 6)   # one hidden layer: the plain network
    assert torch.equal(one(x.float()), torch.nn.Sequential(*one)(x.float()))


def test_c_refusals_name_what_they_refuse_before_any_hip_call():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    fwd = lambda d, o: (L.rlppo_mlp_forward_res(None, N.dims_array(d), len(d) - 1, 0x1000, 0x2000, 16, 4, 0, 0x3000, 32, 0x4000, 1 << 20, ctypes.byref(o)),
                        L.rlppo_last_error().decode())
    o = N.ActOpts()
    o.hidden_act, o.precision = N.ACT_RES, N.PRECISION_BF16   # (with ReLU and no norm: those have refusals of their own, which come first)
    rc, msg = fwd([13, 32, 32, 6], o)
    assert rc == 1001 and "RLPPO_ACT_RES" in msg and "bf16 inference" in msg, msg
    o.hidden_act, o.precision = N.ACT_RES, N.PRECISION_FP32
    rc, msg = fwd([13, 2049, 2049, 6], o)
    assert rc == 1001 and "RLPPO_ACT_RES" in msg and "RLPPO_NORM_MAX_WIDTH = 2048" in msg, msg
    rc, msg = fwd([13, 32, 32, 48, 6], o)
    assert rc == 1001 and "equal hidden widths: hidden layer 2 has 48 outputs" in msg, msg
    rc = L.rlppo_mlp_forward(None, N.dims_array([13, 32, 32, 6]), 3, 0x1000, 0x2000, 16, 4, 0, 0x3000, 32, 0x4000, 1 << 20, ctypes.byref(o))
    assert rc == 1001 and "rlppo_mlp_forward_res" in L.rlppo_last_error().decode()   # the old entry point keeps its contract and names the new one
    o.hidden_act = 0x400
    assert fwd([13, 32, 32, 6], o)[0] == 1001 and "hidden_act 1024" in L.rlppo_last_error().decode()
    assert L.rlppo_row_res_fwd(None, 0x1000, 4096, 0x2000, 4096, 4, 2049, 0, 0x3000, 4096, None, 0) == 1001 and "RLPPO_NORM_MAX_WIDTH = 2048" in L.rlppo_last_error().decode()
    assert L.rlppo_row_res_bwd(None, 0x1000, 32, None, 0, 0x2000, 32, None, 0, 4, 5, 3, 0, None, 0, 0x3000, 32) == 1001 and "act 3" in L.rlppo_last_error().decode()

    def ex(a, **kw):
        e = N.MinibatchExt()
        for k, v in kw.items():
            setattr(e, k, v)
        return L.rlppo_ppo_minibatch_ex(None, ctypes.byref(a), ctypes.byref(e)), L.rlppo_last_error().decode()
    for prec, word in ((N.PRECISION_BF16, "bf16"), (N.PRECISION_X3, "x3")):
        a = _args(N, L, head=0, act_dim=1)
        a.precision = prec
        rc, msg = ex(a, pol_hidden_act=N.ACT_RES)
        assert rc == 1001 and "RLPPO_ACT_RES" in msg and f"update precision {word}" in msg, msg
    # the sizing functions: the old ones answer what they answered, the new ones know the flag
    a = _args(N, L, head=0, act_dim=1)
    sizes = (a.pol_dims, a.pol_layers, a.val_dims, a.val_layers, a.mb, N.PRECISION_FP32)
    old, normed = int(L.rlppo_minibatch_workspace_bytes_for(*sizes)), int(L.rlppo_minibatch_workspace_bytes_norm(*sizes, 0, N.ACT_NORM, 0))
    assert L.rlppo_minibatch_workspace_bytes_norm(*sizes, 0, N.ACT_RES, 0) == 0 and L.rlppo_minibatch_workspace_bytes_res(*sizes, 0, 0x400, 0) == 0
    assert (int(L.rlppo_minibatch_workspace_bytes_res(*sizes, 0, 0, 0)), int(L.rlppo_minibatch_workspace_bytes_res(*sizes, 0, N.ACT_NORM, 0))) == (old, normed)
    assert int(L.rlppo_minibatch_workspace_bytes_res(*sizes, 0, N.ACT_RES | N.ACT_NORM, 0)) > int(L.rlppo_minibatch_workspace_bytes_res(*sizes, 0, N.ACT_RES, 0)) > old
    a.precision, a.ws_bytes = N.PRECISION_FP32, old
    rc, msg = ex(a, pol_hidden_act=N.ACT_RES)
    assert rc == 1002 and "rlppo_minibatch_workspace_bytes_res" in msg, msg
    d3, base = N.dims_array([13, 32, 32, 6]), int(L.rlppo_forward_workspace_bytes(N.dims_array([13, 32, 32, 6]), 3, 64))
    assert [int(L.rlppo_forward_workspace_bytes_act(d3, 3, 64, c)) for c in (0, N.ACT_NORM, N.ACT_RES, 0x400)] == [base, base, base, 0]
    assert int(L.rlppo_forward_workspace_bytes_act(d3, 3, 64, N.ACT_RES | N.ACT_NORM)) - 256 == (base - 256) * 3 // 2
    assert int(L.rlppo_discrete_step_workspace_bytes_act(d3, 3, 64, N.ACT_RES | N.ACT_NORM)) > int(L.rlppo_discrete_step_workspace_bytes(d3, 3, 64))


def test_learner_refusals_and_the_agreement_rule(monkeypatch, tmp_path):
    import synthetic_env
    from rlgym_ppo_amd import engine
    from rlgym_ppo_amd import learner as LM
    from rlgym_ppo_amd.ppo import LayerSizes

    for manager in ("BatchedAgentManager", "VectorAgentManager"):   # (nothing may get as far as building one)
        monkeypatch.setattr(LM, manager, lambda *a, **k: pytest.fail("a refused Learner reached its agent manager"))
    kw = dict(device="cuda:0", checkpoints_save_folder=str(tmp_path / "c"), add_unix_timestamp=False, checkpoint_load_folder=None)
    make = lambda **k: LM.Learner(synthetic_env.make_continuous_wire_env, **k, **kw)
    for text, k in (("hidden_residual must be", dict(hidden_residual="both")),
                    ("critic_layer_sizes.*residual=True.*hidden_residual='policy'", dict(hidden_residual="policy", critic_layer_sizes=LayerSizes((8, 8), residual=True))),
                    ("equal hidden widths: hidden layer 1 has 128", dict(hidden_residual="critic", critic_layer_sizes=(256, 128)))):
        with pytest.raises(ValueError, match=text):
            make(**k)
    for setter, mode, word in ((engine.set_update_precision, "bf16", "update precision 'bf16'"), (engine.set_update_precision, "x3", "update precision 'x3'"),
                               (engine.set_inference_precision, "bf16", "bf16 inference precision")):
        setter(mode)
        try:
            with pytest.raises(ValueError, match=f"hidden_residual.*{word}"):
                make(hidden_residual=True)
        finally:
            setter("fp32")
