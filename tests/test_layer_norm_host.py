"""CPU checks of hidden layer normalisation (ppo.LayerSizes(..., norm="layer"), Learner(hidden_layer_norm=...); include/rlppo.h,
"[norm]"): the tuple, the torch module, and the refusals -- the C-level ones on a null stream with placeholder pointers, so they
come before any HIP call.  No GPU."""
import ctypes
import pickle

import pytest
import torch
import torch.nn.functional as F

from test_diag_gaussian_host import _args  # placeholder arguments of a pass


def test_layer_sizes_round_trip():
    from rlgym_ppo_amd.ppo import LayerSizes
    ls = LayerSizes((64, 32), "tanh", "layer")
    back = pickle.loads(pickle.dumps(ls))
    assert isinstance(ls, tuple) and ls == (64, 32) and (back, back.activation, back.norm) == (ls, "tanh", "layer")
    assert LayerSizes((8,)).norm is None and LayerSizes((8,), "elu").norm is None and LayerSizes(ls, norm=ls.norm).norm == "layer"
    assert eval(repr(ls)).norm == "layer" and repr(LayerSizes((8,), "elu")) == "LayerSizes((8,), 'elu')"
    with pytest.raises(ValueError, match="hidden normalisation"):
        LayerSizes((8,), "relu", "batch")


@pytest.mark.parametrize("act", ["relu", "tanh", "elu"])
def test_build_body_is_layer_norm_of_the_activation_on_the_same_weights(act):
    from rlgym_ppo_amd.ppo import LayerSizes
    from rlgym_ppo_amd.ppo._mlp import activation_of, build_body, norm_of
    torch.manual_seed(3)
    plain = build_body(13, LayerSizes((32, 48), act), 6)
    torch.manual_seed(3)
    body = build_body(13, LayerSizes((32, 48), act, "layer"), 6).double()
    sd, ref = body.state_dict(), plain.state_dict()
    assert list(sd) == list(ref) and all(torch.equal(sd[k].float(), ref[k]) for k in ref)
    assert (activation_of(body), norm_of(body), norm_of(plain)) == (act, "layer", None) and len(body) == len(plain)
    x = torch.randn(7, 13, dtype=torch.float64)
    want = x
    for i, w in ((0, 32), (2, 48)):
        want = F.layer_norm(getattr(F, act)(body[i](want)), (w,), eps=1e-5)
    assert torch.equal(body(x), body[4](want))


def test_c_refusals_name_what_they_refuse_before_any_hip_call():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    dims, wide = N.dims_array([13, 32, 32, 6]), N.dims_array([13, 2049, 6])
    fwd = lambda d, nl, o: (L.rlppo_mlp_forward(None, d, nl, 0x1000, 0x2000, 16, 4, 0, 0x3000, 32, 0x4000, 1 << 20, ctypes.byref(o)),
                            L.rlppo_last_error().decode())
    o = N.ActOpts()
    for bad in (3, 7, -1, 0x103, 0x200):                          # what was refused stays refused, with its text
        o.hidden_act = bad
        rc, msg = fwd(dims, 3, o)
        assert rc == 1001 and f"hidden_act {bad}" in msg and "2 = ELU" in msg, msg
    o.hidden_act, o.precision = N.ACT_NORM, N.PRECISION_BF16   # (with ReLU: tanh / ELU already have a refusal of their own)
    rc, msg = fwd(dims, 3, o)
    assert rc == 1001 and "normalisation" in msg and "bf16 inference" in msg, msg
    o.precision = N.PRECISION_FP32
    rc, msg = fwd(wide, 2, o)
    assert rc == 1001 and "RLPPO_NORM_MAX_WIDTH = 2048" in msg, msg
    assert L.rlppo_row_norm_fwd(None, 0x1000, 4096, 4, 2049, 0x2000, 4096) == 1001 and "RLPPO_NORM_MAX_WIDTH = 2048" in L.rlppo_last_error().decode()
    assert L.rlppo_row_norm_bwd(None, 0x1000, 32, 0x2000, 32, 4, 5, 3, 0x3000, 32) == 1001 and "act 3" in L.rlppo_last_error().decode()

    def ex(a, **kw):
        e = N.MinibatchExt()
        for k, v in kw.items():
            setattr(e, k, v)
        return L.rlppo_ppo_minibatch_ex(None, ctypes.byref(a), ctypes.byref(e)), L.rlppo_last_error().decode()
    for prec, word in ((N.PRECISION_BF16, "bf16"), (N.PRECISION_X3, "x3")):
        a = _args(N, L, head=0, act_dim=1)
        a.precision = prec
        rc, msg = ex(a, val_hidden_act=N.ACT_NORM)
        assert rc == 1001 and "normalisation" in msg and f"update precision {word}" in msg, msg
    for kw in ({"pol_hidden_act": 3}, {"val_hidden_act": -1}, {"pol_hidden_act": 7, "val_hidden_act": 0x100}):
        rc, msg = ex(_args(N, L, head=0, act_dim=1), **kw)
        assert rc == 1001 and "hidden_act" in msg and "2 = ELU" in msg, msg
    # a workspace sized by the function that never heard of the option: too small, and the message names the one that has
    a = _args(N, L, head=0, act_dim=1)
    sizes = (a.pol_dims, a.pol_layers, a.val_dims, a.val_layers, a.mb, N.PRECISION_FP32)
    old, new = int(L.rlppo_minibatch_workspace_bytes_for(*sizes)), int(L.rlppo_minibatch_workspace_bytes_norm(*sizes, 0, N.ACT_NORM, 0))
    assert new > old == int(L.rlppo_minibatch_workspace_bytes_norm(*sizes, 0, 0, 2)) and L.rlppo_minibatch_workspace_bytes_norm(*sizes, 0, 3, 0) == 0
    a.precision, a.ws_bytes = N.PRECISION_FP32, old
    rc, msg = ex(a, pol_hidden_act=N.ACT_NORM)
    assert rc == 1002 and "rlppo_minibatch_workspace_bytes_norm" in msg, msg


def test_learner_refusals_come_before_anything_is_built(monkeypatch, tmp_path):
    import synthetic_env
    from rlgym_ppo_amd import engine
    from rlgym_ppo_amd import learner as LM
    from rlgym_ppo_amd.ppo import LayerSizes

    class Reached(Exception):
        pass

    def never(*a, **k):
        raise Reached()
    monkeypatch.setattr(LM, "BatchedAgentManager", never)
    monkeypatch.setattr(LM, "VectorAgentManager", never)
    kw = dict(device="cuda:0", checkpoints_save_folder=str(tmp_path / "c"), add_unix_timestamp=False, checkpoint_load_folder=None)
    make = lambda **k: LM.Learner(synthetic_env.make_continuous_wire_env, **k, **kw)
    with pytest.raises(ValueError, match="hidden_layer_norm must be"):
        make(hidden_layer_norm="batch")
    with pytest.raises(ValueError, match="critic_layer_sizes.*norm='layer'.*hidden_layer_norm='policy'"):
        make(hidden_layer_norm="policy", critic_layer_sizes=LayerSizes((8,), norm="layer"))
    for setter, mode, word in ((engine.set_update_precision, "bf16", "update precision 'bf16'"), (engine.set_update_precision, "x3", "update precision 'x3'"),
                               (engine.set_inference_precision, "bf16", "bf16 inference precision")):
        setter(mode)
        try:
            with pytest.raises(ValueError, match=f"hidden_layer_norm.*{word}"):
                make(hidden_layer_norm=True)
        finally:
            setter("fp32")
