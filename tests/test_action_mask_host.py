"""Invalid-action masking, the parts that need no GPU: the pack / unpack helper against a numpy restatement of the encoding
(uint32 words, W = ceil(A / 32) per row, bit c % 32 of word c / 32 set = action c valid, bits beyond A clear), and the argument
checks of rlppo_ppo_minibatch (a mask with a head other than the discrete one, a wrong mask_words: 1001 with a message naming the
field, before any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch


def restate(mask):
    """The encoding, bit by bit."""
    n, A = mask.shape
    W = (A + 31) // 32
    out = np.zeros((n, W), np.uint64)
    for r in range(n):
        for c in range(A):
            if mask[r, c]:
                out[r, c // 32] |= np.uint64(1) << np.uint64(c % 32)
    return out.astype(np.uint32)


@pytest.mark.parametrize("A", [1, 3, 31, 32, 33, 90, 128, 200, 2048])
def test_pack_unpack_against_numpy_restatement(A):
    from rlgym_ppo_amd.util import action_mask as AM
    rs = np.random.RandomState(A)
    n = 37
    m = rs.rand(n, A) < 0.6
    m[np.arange(n), rs.randint(0, A, n)] = True   # every row has a valid action
    m[3] = True                                   # a row all valid
    m[5] = False
    m[5, A - 1] = True                            # a row with exactly one valid action: the last
    want = restate(m)
    assert AM.mask_words(A) == want.shape[1] == (A + 31) // 32
    for form in (m, m.astype(np.float32), m.astype(np.int64), torch.from_numpy(m), m.tolist()):
        got = AM.pack(form, A, "cpu")
        assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
        assert np.array_equal(got.numpy().view(np.uint32), want), A
    # bits at and beyond A are clear
    if A % 32:
        assert (want[:, -1] >> np.uint32(A % 32)).max() == 0
    back = AM.unpack(AM.pack(m, A, "cpu"), A)
    assert back.dtype == torch.bool and np.array_equal(back.numpy(), m)
    packed = AM.Packed(AM.pack(m, A, "cpu"), A)
    assert AM.pack(packed, A, "cpu") is not None and np.array_equal(packed.unpack().numpy(), m) and packed.shape == (n, A)


def test_empty_host_row_raises_and_names_the_row():
    from rlgym_ppo_amd.util import action_mask as AM
    m = np.ones((9, 90), bool)
    m[6] = False
    with pytest.raises(ValueError, match="row 6"):
        AM.pack(m, 90, "cpu")
    with pytest.raises(ValueError, match="row 6"):
        AM.pack(torch.from_numpy(m), 90, "cpu")
    with pytest.raises(ValueError, match="shape"):
        AM.pack(np.ones((9, 89), bool), 90, "cpu")


def test_structs_carry_the_mask_fields_and_abi_is_8():
    from rlgym_ppo_amd import _native as N
    assert N.ABI_VERSION == 8 and N.lib().rlppo_abi_version() == 8
    assert [f[0] for f in N.ActOpts._fields_][-2:] == ["action_mask", "mask_words"]
    assert [f[0] for f in N.MinibatchArgs._fields_][-2:] == ["action_mask", "mask_words"]


def test_ppo_minibatch_rejects_a_mask_it_cannot_take_before_any_launch():
    """Placeholder pointers, no GPU: the checks run before the first HIP call."""
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    val = N.dims_array([107, 256, 256, 256, 1])

    def call(head, n_out, act_dim, mask_words, mask=True):
        pol = N.dims_array([107, 256, 256, 256, n_out])
        a = N.MinibatchArgs()
        a.head, a.pol_layers, a.val_layers, a.act_dim, a.slot, a.precision = head, 4, 4, act_dim, 0, N.PRECISION_FP32
        a.pol_dims = ctypes.cast(pol, ctypes.POINTER(ctypes.c_int32))
        a.val_dims = ctypes.cast(val, ctypes.POINTER(ctypes.c_int32))
        fake = iter(range(0x10000, 0x1000000, 0x1000))  # distinct, never dereferenced
        for f in ("pol_packed", "val_packed", "pol_grad", "val_grad", "states", "actions", "old_logp", "targets", "advantages", "idx",
                  "stats", "workspace"):
            setattr(a, f, next(fake))
        if mask:
            a.action_mask = next(fake)
        a.mask_words = mask_words
        a.ld_states, a.n_rows, a.mb = 112, 5000, 1500
        a.clip_range, a.ent_coef, a.mb_ratio, a.var_m, a.var_b = 0.2, 0.005, 1.0, 1.0, 0.0
        a.ws_bytes = L.rlppo_minibatch_workspace_bytes_for(pol, 4, val, 4, a.mb, N.PRECISION_FP32)
        assert a.ws_bytes > 0
        return L.rlppo_ppo_minibatch(None, ctypes.byref(a)), L.rlppo_last_error().decode()

    rc, msg = call(N.HEAD_GAUSSIAN, 16, 8, 1)
    assert rc == 1001 and "action_mask" in msg and "Gaussian" in msg, (rc, msg)
    rc, msg = call(N.HEAD_MULTIDISCRETE, 21, 8, 1)
    assert rc == 1001 and "action_mask" in msg and "multi-discrete" in msg, (rc, msg)
    for bad in (0, 2, 4):
        rc, msg = call(N.HEAD_DISCRETE, 90, 1, bad)
        assert rc == 1001 and "mask_words" in msg and "3" in msg, (rc, msg)
    rc, msg = call(N.HEAD_DISCRETE, 200, 1, 3)
    assert rc == 1001 and "mask_words" in msg, (rc, msg)


def test_other_heads_reject_the_argument_in_python():
    """The signatures keep the reference's as a prefix; the two other policy classes refuse a mask by name."""
    import inspect
    from rlgym_ppo_amd.ppo.continuous_policy import ContinuousPolicy
    from rlgym_ppo_amd.ppo.discrete_policy import DiscreteFF
    from rlgym_ppo_amd.ppo.multi_discrete_policy import MultiDiscreteFF
    for cls in (DiscreteFF, ContinuousPolicy, MultiDiscreteFF):
        for name in ("get_action", "act_padded", "get_output", "get_backprop_data"):
            ps = list(inspect.signature(getattr(cls, name)).parameters.values())
            assert ps[-1].name == "action_mask" and ps[-1].default is None, (cls, name)
    assert list(inspect.signature(DiscreteFF.get_action).parameters)[:5] == ["self", "obs", "deterministic", "noise", "standardize"]
    for cls, head in ((ContinuousPolicy, "Gaussian"), (MultiDiscreteFF, "multi-discrete")):
        with pytest.raises(ValueError, match=head):
            cls.get_output(object.__new__(cls), None, action_mask=np.ones((1, 3)))
