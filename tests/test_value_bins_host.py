"""CPU checks of the categorical critic (ppo.ValueBins, LayerSizes(..., value_head=...), Learner(ppo_value_head=...); include/rlppo.h,
"[vbins]"): the record, the tuple, the torch module, and the refusals -- the C-level ones on a null stream with placeholder pointers,
so they come before any HIP call.  No GPU."""
import ctypes
import pickle

import pytest
import torch

from test_diag_gaussian_host import _args  # placeholder arguments of a pass


@pytest.mark.parametrize("kw, word", [(dict(n=1), "n must be"), (dict(n=257), "n must be"), (dict(n=8.5), "n must be"), (dict(kind="c51"), "kind"),
                                      (dict(value_range=(1.0, 1.0)), "vmin < vmax"), (dict(value_range=(0.0, float("inf"))), "finite"),
                                      (dict(value_range=3.0), "pair"), (dict(sigma_ratio=0.0), "sigma_ratio"), (dict(sigma_ratio=2.5), "sigma_ratio")])
def test_value_bins_validation(kw, word):
    from rlgym_ppo_amd.ppo import ValueBins
    with pytest.raises(ValueError, match=word):
        ValueBins(**kw)
    b = ValueBins()
    assert (b.n, b.value_range, b.kind, b.sigma_ratio) == (101, (-10.0, 10.0), "hl_gauss", 0.75) and eval(repr(b)) == b == pickle.loads(pickle.dumps(b))
    arg = ValueBins(9, (-1, 3), "two_hot").c_arg()
    assert (arg.kind, arg.n, arg.vmin, arg.vmax) == (2, 9, -1.0, 3.0)


def test_layer_sizes_round_trip_and_the_modules_built():
    from rlgym_ppo_amd.ppo import LayerSizes, ValueBins
    from rlgym_ppo_amd.ppo._mlp import build_body
    ls = LayerSizes((64, 32), "tanh", None, ValueBins(51))
    back = pickle.loads(pickle.dumps(ls))
    assert tuple(ls) == (64, 32) and (back, back.activation, back.norm, back.value_head) == (ls, "tanh", None, ValueBins(51))
    assert eval(repr(ls)).value_head == ValueBins(51) and LayerSizes((8,)).value_head is None and repr(LayerSizes((8,), "elu")) == "LayerSizes((8,), 'elu')"
    with pytest.raises(ValueError, match="value_head must be"):
        LayerSizes((8,), value_head=51)
    with pytest.raises(ValueError, match="value_head.*policy"):
        build_body(13, ls, 6)
    # "scalar" builds what was built before: the same modules, the same state_dict keys, the same draws
    torch.manual_seed(3)
    old = build_body(13, (32, 48), 1)
    torch.manual_seed(3)
    new, cat = build_body(13, LayerSizes((32, 48)), 1, critic=True), build_body(13, LayerSizes((32, 48), value_head=ValueBins(51)), 51, critic=True)
    assert [type(m) for m in new] == [type(m) for m in old] and all(torch.equal(a, b) for a, b in zip(new.state_dict().values(), old.state_dict().values()))
    assert list(cat.state_dict()) == list(old.state_dict()) and cat[-1].weight.shape == (51, 48)


def test_abi_has_the_added_entry_points():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    assert L.rlppo_abi_version() == 8 and all(hasattr(L, name) for name in ("rlppo_value_bins_readout", "rlppo_ppo_minibatch_vbins"))
    assert ctypes.sizeof(N.ValueBinsArg) == 20 and L.rlppo_dbg_counter(N.COUNTER_VBINS_PASS) >= 0   # (a known key: unknown ones answer -1)


BINS = dict(kind=1, n=9, vmin=-1.0, vmax=1.0, sigma_ratio=0.75)


@pytest.mark.parametrize("bins, args, word", [
    (dict(n=1), {}, "n=1"), (dict(n=257), {}, "n=257"), (dict(n=8), {}, "bins n=8, but the critic has 9 outputs"), (dict(vmin=1.0), {}, "vmin=1 vmax=1"),
    (dict(vmax=float("nan")), {}, "vmax=nan"), (dict(sigma_ratio=0.0), {}, "sigma_ratio=0"), (dict(sigma_ratio=2.5), {}, "sigma_ratio=2.5"),
    (dict(sigma_ratio=1e-44), {}, "1 / sigma is not a float32"), (dict(kind=3), {}, "kind=3"), ({}, dict(value_clip=0.2), "value_clip=0.2"), ({}, dict(precision=2), "update precision bf16"),
    ({}, dict(precision=3), "update precision x3")])
def test_c_refusals_name_what_they_refuse_before_any_hip_call(bins, args, word):
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    a = _args(N, L, head=0, act_dim=1, pol=[107, 64, 6], val=[107, 64, 9])
    for k, v in args.items():
        setattr(a, k, v)
    b = N.ValueBinsArg(**dict(BINS, **bins))
    before = [L.rlppo_dbg_counter(k) for k in (2, 17)]
    assert L.rlppo_ppo_minibatch_vbins(None, ctypes.byref(a), None, None, None, ctypes.byref(b)) == 1001
    msg = L.rlppo_last_error().decode()
    assert "ppo_minibatch_vbins" in msg and word in msg, msg
    if not args and "critic has" not in word:   # the readout refuses the same bins
        assert L.rlppo_value_bins_readout(None, 0x1000, 32, ctypes.byref(b), 0x2000, 4) == 1001 and word in L.rlppo_last_error().decode()
    assert [L.rlppo_dbg_counter(k) for k in (2, 17)] == before
    assert L.rlppo_value_bins_readout(None, 0x1000, 36, ctypes.byref(N.ValueBinsArg(**BINS)), 0x2000, 4) == 1001   # rows of no multiple of 8 floats


def test_learner_refusals_come_before_anything_is_built(monkeypatch, tmp_path):
    import synthetic_env
    from rlgym_ppo_amd import engine
    from rlgym_ppo_amd import learner as LM
    from rlgym_ppo_amd.ppo import LayerSizes, ValueBins

    def never(*a, **k):
        raise AssertionError("a manager was built")
    monkeypatch.setattr(LM, "BatchedAgentManager", never)
    monkeypatch.setattr(LM, "VectorAgentManager", never)
    kw = dict(device="cuda:0", checkpoints_save_folder=str(tmp_path / "c"), add_unix_timestamp=False, checkpoint_load_folder=None)
    make = lambda **k: LM.Learner(synthetic_env.make_discrete_env, **k, **kw)
    own = LayerSizes((8,), value_head=ValueBins(9))
    for k, word in ((dict(ppo_value_head="c51"), "ppo_value_head must be"), (dict(ppo_value_head="two_hot", ppo_value_bins=1), "n must be"),
                    (dict(ppo_value_head="hl_gauss", ppo_value_clip_range=0.2), "ppo_value_clip_range=0.2"),
                    (dict(critic_layer_sizes=own, ppo_value_clip_range=0.2), "ppo_value_clip_range=0.2"),
                    (dict(ppo_value_head="hl_gauss", ppo_normalize_value=True, ppo_value_norm_popart=True), "ppo_value_norm_popart=True"),
                    (dict(ppo_value_head="hl_gauss", critic_layer_sizes=own), "give one of them"), (dict(policy_layer_sizes=own), "policy_layer_sizes")):
        with pytest.raises(ValueError, match=word):
            make(ppo_normalize_value=k.pop("ppo_normalize_value", True), **k)
    for mode in ("bf16", "x3"):
        engine.set_update_precision(mode)
        try:
            with pytest.raises(ValueError, match=f"ppo_value_head.*update precision '{mode}'"):
                make(ppo_value_head="two_hot", ppo_normalize_value=True)
        finally:
            engine.set_update_precision("fp32")
    # accepted (and warned about: real value units, the default range) -- the constructor goes on to the device or the manager
    with pytest.warns(RuntimeWarning, match="ppo_value_range is in real value units"), pytest.raises(Exception):
        make(ppo_value_head="hl_gauss")
