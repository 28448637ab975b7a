"""CPU checks of the hidden-activation choice (Learner(hidden_activation=...), ppo.LayerSizes; include/rlppo.h, "[act]"): the
LayerSizes tuple, build_body for the three activations, the Learner's refusals before anything is built, the agreement of the
header and the ctypes table, and the argument errors of the C boundary that need no device.  No GPU, no compute call.

rlppo_act_opts.hidden_act lives in the struct's 4 bytes of tail padding.  The struct is {int32, uint32, 3 pointers, int32}: its size is
40 bytes and the padding sits at offset 36 (include/rlppo.h asserts both), so those are the numbers pinned here -- a member at
offset 44 of a 48-byte struct would have GROWN the struct and made the library read past the 40 bytes an ABI-8 caller passes."""
import ctypes
import inspect
import pickle

import pytest
import torch

import synthetic_env
from test_diag_gaussian_host import _Agent, _args, _learner  # the monkeypatched stand-ins / placeholder arguments

ACTS = ("relu", "tanh", "elu")


def test_layer_sizes_is_a_tuple_that_carries_the_activation():
    from rlgym_ppo_amd.ppo import LayerSizes
    ls = LayerSizes((64, 32), "tanh")
    assert isinstance(ls, tuple) and ls == (64, 32) and tuple(ls) == (64, 32) and type(tuple(ls)) is tuple
    assert len(ls) == 2 and ls[0] == 64 and list(ls[1:]) == [32] and ls.activation == "tanh"
    assert LayerSizes([256, 256, 256]).activation == "relu" and LayerSizes((8,), activation="elu").activation == "elu"
    assert LayerSizes(ls, "tanh").activation == "tanh"
    back = pickle.loads(pickle.dumps(ls))
    assert type(back) is LayerSizes and back == ls and back.activation == "tanh"
    for bad in ("gelu", "ReLU", "", None, 1):
        with pytest.raises(ValueError, match="hidden activation"):
            LayerSizes((64, 64), bad)


def test_build_body_same_keys_same_weights_right_modules():
    from rlgym_ppo_amd.ppo import LayerSizes
    from rlgym_ppo_amd.ppo._mlp import activation_of, build_body
    want = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "elu": torch.nn.ELU}
    bodies = {}
    for act in ACTS:
        torch.manual_seed(11)
        bodies[act] = build_body(13, LayerSizes((32, 48, 16), act), 6, torch.nn.Softmax(dim=-1))
        after = torch.rand(1).item()   # the generator's position after construction
        torch.manual_seed(11)
        plain = build_body(13, (32, 48, 16), 6, torch.nn.Softmax(dim=-1))
        assert torch.rand(1).item() == after, "the activation changed what the CPU generator was asked for"
        assert all(type(m) is torch.nn.ReLU for m in list(plain)[1:6:2])   # a plain tuple is ReLU, as it always was
    ref = bodies["relu"].state_dict()
    assert list(ref) == [f"{i}.{p}" for i in (0, 2, 4, 6) for p in ("weight", "bias")]
    for act in ACTS:
        body, sd = bodies[act], bodies[act].state_dict()
        assert list(sd) == list(ref) and all(sd[k].shape == ref[k].shape and torch.equal(sd[k], ref[k]) for k in ref), act
        assert [type(m) for m in list(body)[1:6:2]] == [want[act]] * 3 and type(body[7]) is torch.nn.Softmax and len(body) == 8
        assert activation_of(body) == act
        if act == "elu":
            assert body[1].alpha == 1.0
    with pytest.raises(ValueError, match="hidden activation"):
        ls = LayerSizes((8, 8))
        ls.activation = "swish"
        build_body(4, ls, 2)


def test_learner_refuses_before_anything_is_built(monkeypatch, tmp_path):
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd import learner as LM
    from rlgym_ppo_amd.ppo import LayerSizes
    ps = inspect.signature(Learner.__init__).parameters
    names = list(ps)
    assert ps["hidden_activation"].default == "relu" and names[names.index("hidden_activation") - 1] == "continuous_action_clip"

    def never(*a, **k):
        raise AssertionError("the refusal must come before the collection manager is built")
    monkeypatch.setattr(LM, "BatchedAgentManager", never)
    monkeypatch.setattr(LM, "VectorAgentManager", never)
    kw = dict(device="cuda:0", checkpoints_save_folder=str(tmp_path / "c"), add_unix_timestamp=False, checkpoint_load_folder=None)
    with pytest.raises(ValueError, match="hidden activation.*'gelu'"):
        LM.Learner(synthetic_env.make_continuous_wire_env, hidden_activation="gelu", **kw)
    for arg in ("policy_layer_sizes", "critic_layer_sizes"):
        with pytest.raises(ValueError, match=f"{arg}.*'elu'.*hidden_activation='tanh'"):
            LM.Learner(synthetic_env.make_continuous_wire_env, hidden_activation="tanh", **{arg: LayerSizes((32, 32), "elu")}, **kw)

    # what reaches PPOLearner: both size arguments wrapped; a LayerSizes wins while hidden_activation is left at its default
    class Reached(Exception):
        pass

    def stand_in(*a, **k):
        raise Reached(k["policy_layer_sizes"], k["critic_layer_sizes"])
    monkeypatch.setattr(LM, "PPOLearner", stand_in)
    for extra, want in (({}, ("relu", "relu")), ({"hidden_activation": "elu"}, ("elu", "elu")),
                        ({"policy_layer_sizes": LayerSizes((32, 32), "tanh")}, ("tanh", "relu")),
                        # (the documented exception: the default IS "relu", so an explicit "relu" cannot be told from an omitted one)
                        ({"hidden_activation": "relu", "policy_layer_sizes": LayerSizes((32, 32), "tanh")}, ("tanh", "relu")),
                        ({"hidden_activation": "tanh", "critic_layer_sizes": LayerSizes((16,), "tanh")}, ("tanh", "tanh"))):
        with pytest.raises(Reached) as reached:
            _learner(monkeypatch, tmp_path, **extra)
        pol, val = reached.value.args
        assert type(pol) is LayerSizes and type(val) is LayerSizes and (pol.activation, val.activation) == want, extra
        assert tuple(pol) == tuple(extra.get("policy_layer_sizes", (256, 256, 256))) and tuple(val) == tuple(extra.get("critic_layer_sizes", (256, 256, 256)))
    assert _Agent.code == 2


def test_header_and_ctypes_agree_on_the_new_members():
    from rlgym_ppo_amd import _native as N
    header = open(N.HERE + "/../include/rlppo.h").read()
    assert ctypes.sizeof(N.ActOpts) == 40 and N.ActOpts.hidden_act.offset == 36 and N.ActOpts.hidden_act.size == 4
    assert N.ActOpts.mask_words.offset == 32   # the member fills the tail padding behind mask_words
    assert "sizeof(rlppo_act_opts) == 40 && offsetof(rlppo_act_opts, hidden_act) == 36" in header
    body = header[header.index("typedef struct rlppo_act_opts {"):header.index("} rlppo_act_opts;")]
    assert body.rstrip().endswith("int32_t hidden_act;")
    o = N.ActOpts(N.PRECISION_DEFAULT, 1, None)
    assert o.hidden_act == 0 and bytes(o) == bytes(N.ActOpts(N.PRECISION_DEFAULT, 1, None))   # a fresh struct is zero-filled: ReLU
    o.hidden_act = 2
    assert o.hidden_act == 2 and o.mask_words == 0 and bytes(o)[36:40] == (2).to_bytes(4, "little")
    assert (N.ACT_RELU, N.ACT_TANH, N.ACT_ELU) == (0, 1, 2) and N.HIDDEN_ACTIVATIONS == {"relu": 0, "tanh": 1, "elu": 2}
    for name, code in (("RELU", 0), ("TANH", 1), ("ELU", 2)):
        assert f"#define RLPPO_ACT_{name} {code}" in header
    assert "int rlppo_ppo_minibatch_ex(void *stream, const rlppo_minibatch_args *args, const rlppo_minibatch_ext *ext);" in header
    assert N.SIGNATURES["rlppo_ppo_minibatch_ex"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(N.MinibatchArgs), ctypes.POINTER(N.MinibatchExt)])
    assert hasattr(N.lib(), "rlppo_ppo_minibatch_ex")
    ext = header[header.index("typedef struct rlppo_minibatch_ext {"):header.index("} rlppo_minibatch_ext;")]
    fields = []
    for decl in ext.split("{")[1].split(";")[:-1]:
        fields += [part.replace("*", " ").split()[-1] for part in decl.split(",")]
    assert fields == [f[0] for f in N.MinibatchExt._fields_]
    assert ctypes.sizeof(N.MinibatchExt) == 56
    assert N.ABI_VERSION == 8 and "#define RLPPO_ABI_VERSION 8" in header
    assert "4 bias+ELU" in header and "5 times tanh'" in header and "6 times ELU'" in header   # rlppo_dbg_gemm_nt's comment


def test_act_options_refuse_an_unknown_activation_before_any_hip_call():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    dims = N.dims_array([13, 32, 32, 6])
    o = N.ActOpts()
    o.hidden_act = 7
    calls = {
        "mlp_forward": lambda: L.rlppo_mlp_forward(None, dims, 3, 0x1000, 0x2000, 16, 4, 0, 0x3000, 32, 0x4000, 1 << 20, ctypes.byref(o)),
        "discrete_act": lambda: L.rlppo_discrete_act(None, dims, 3, 0x1000, 0x2000, 16, 4, 0x3000, 0x4000, 0x5000, None, 0x6000, 1 << 20, ctypes.byref(o)),
        "discrete_step": lambda: L.rlppo_discrete_step(None, dims, 3, 0x1000, 0x2000, 0, 13, 4, 0, 0.0, 1.0, None, None, 0x3000, 0x4000, None, 0x5000,
                                                       None, 0, 0x6000, 1 << 20, ctypes.byref(o)),
        "discrete_probs": lambda: L.rlppo_discrete_probs(None, dims, 3, 0x1000, 0x2000, 16, 4, 0, 0x3000, 6, None, 0x4000, 1 << 20, ctypes.byref(o)),
        "gaussian_act": lambda: L.rlppo_gaussian_act(None, dims, 3, 0x1000, 0x2000, 16, 4, 0x3000, 0.45, 0.55, 0x4000, 0x5000, 0x6000, 1 << 20,
                                                     ctypes.byref(o)),
        "diag_gaussian_act": lambda: L.rlppo_diag_gaussian_act(None, dims, 3, 0x1000, 0x2000, 16, 4, 0x3000, 0x3800, 0x4000, 0x5000, 0x6000, 1 << 20,
                                                               ctypes.byref(o)),
        "multidiscrete_act_nvec": lambda: L.rlppo_multidiscrete_act_nvec(None, dims, 3, 0x1000, 0x2000, 16, 4, 0x3000, 0x4000, 0x5000, 0x6000, 1 << 20,
                                                                         ctypes.byref(o), N.dims_array([2, 4]), 2),
    }
    for name, call in calls.items():
        rc, msg = call(), L.rlppo_last_error().decode()
        assert rc == 1001 and "hidden_act 7" in msg and "tanh" in msg, (name, rc, msg)
    assert L.rlppo_discrete_step_one_launch(dims, 3, 4, ctypes.byref(o)) == -1
    # tanh / ELU: no bf16 inference precision (that rlppo_discrete_step_one_launch answers 0 for them needs the device's answer for
    # ReLU beside it: tests/test_gpu_hidden_activation.py)
    for code, name in ((1, "tanh"), (2, "elu")):
        o = N.ActOpts()
        o.hidden_act = code
        o.precision = N.PRECISION_BF16
        rc = L.rlppo_mlp_forward(None, dims, 3, 0x1000, 0x2000, 16, 4, 0, 0x3000, 32, 0x4000, 1 << 20, ctypes.byref(o))
        msg = L.rlppo_last_error().decode()
        assert rc == 1001 and name in msg and "bf16" in msg, (rc, msg)
    z = N.ActOpts()
    assert L.rlppo_mlp_forward(None, dims, 3, 0x1000, 0x2000, 16, 0, 0, 0x3000, 32, 0x4000, 1 << 20, ctypes.byref(z)) == 0   # (n = 0: no launch)


def test_minibatch_ex_refusals_come_before_any_hip_call():
    from rlgym_ppo_amd import _native as N
    L = N.lib()

    def ex(a, **kw):
        e = N.MinibatchExt()
        for k, v in kw.items():
            setattr(e, k, v)
        return L.rlppo_ppo_minibatch_ex(None, ctypes.byref(a), ctypes.byref(e)), L.rlppo_last_error().decode()

    for prec, word in ((N.PRECISION_BF16, "bf16"), (N.PRECISION_X3, "x3")):
        for kw, name in (({"pol_hidden_act": 1}, "tanh"), ({"val_hidden_act": 2}, "elu"), ({"pol_hidden_act": 2, "val_hidden_act": 1}, "elu")):
            a = _args(N, L, head=0, act_dim=1)
            a.precision = prec
            rc, msg = ex(a, **kw)
            assert rc == 1001 and f"hidden activation {name}" in msg and word in msg, (rc, msg)
    for kw in ({"pol_hidden_act": 3}, {"val_hidden_act": -1}, {"pol_hidden_act": 7, "val_hidden_act": 1}):
        rc, msg = ex(_args(N, L, head=0, act_dim=1), **kw)
        assert rc == 1001 and "hidden_act" in msg and "2 = ELU" in msg, (rc, msg)
    # the extension carries what the other entry points carry: their checks, their messages
    rc, msg = ex(_args(N, L), pol_hidden_act=1)                      # head 3 without log_std
    assert rc == 1001 and "head 3" in msg and "log_std" in msg, (rc, msg)
    rc, msg = ex(_args(N, L), pol_hidden_act=1, log_std=0x2000000, log_std_grad=0x2001000, scratch=0x2002004, scratch_bytes=1 << 20)
    assert rc == 1001 and "scratch" in msg and "aligned" in msg, (rc, msg)
    nvec = N.dims_array([2, 4])
    rc, msg = ex(_args(N, L, head=0, act_dim=1), val_hidden_act=2, md_nvec=ctypes.cast(nvec, ctypes.POINTER(ctypes.c_int32)), md_heads=2)
    assert rc == 1001 and "md_nvec is an option of the multi-discrete head" in msg, (rc, msg)
    a = _args(N, L, head=0, act_dim=1)
    a.mb = 0
    assert ex(a, pol_hidden_act=1)[0] == 0 and L.rlppo_ppo_minibatch_ex(None, ctypes.byref(a), None) == 0   # an empty pass: no error, no launch


def test_ppo_learner_names_activation_and_precision():
    """PPOLearner._check_options (the first thing learn() does) on a stand-in that holds only what the check reads."""
    from rlgym_ppo_amd.ppo import PPOLearner

    class Net:
        def __init__(self, act):
            self.hidden_activation = act

    class Opt:
        param_groups = [{"lr": 3e-4}]

    def learner(pol, val, prec):
        s = object.__new__(PPOLearner)
        s.policy, s.value_net, s.update_precision = Net(pol), Net(val), prec
        s.lr_schedule, s.desired_kl, s.lr_bounds = "constant", 0.01, (1e-5, 1e-2)
        s.policy_optimizer = s.value_optimizer = Opt()
        s.fused_optimizer_step, s.value_clip_range, s.target_kl, s.max_grad_norm = True, None, None, 0.5
        return s
    for prec in ("bf16", "x3"):
        for pol, val, name in (("tanh", "tanh", "tanh"), ("relu", "elu", "elu")):
            with pytest.raises(ValueError, match=f"hidden activation '{name}'.*update precision '{prec}'"):
                learner(pol, val, prec)._check_options()
        learner("relu", "relu", prec)._check_options()
    learner("tanh", "elu", "fp32")._check_options()
    learner("elu", "elu", None)._check_options()   # (the process default is fp32)
