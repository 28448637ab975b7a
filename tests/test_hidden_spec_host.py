"""The workspace sizes of the wide forms equal those of the narrow ones wherever the bits they add are absent, on the CPU: what lets
NetArena and PPOLearner always call the widest form (rlppo_forward_workspace_bytes_act, rlppo_discrete_step_workspace_bytes_act,
rlppo_minibatch_workspace_bytes_res) whatever the networks' hidden layers are."""
import itertools

from rlgym_ppo_amd import _native as N

DIMS = ([7, 8, 3], [107, 128, 128, 90], [13, 64, 64, 64, 1], [5, 256, 1])
ROWS = (0, 1, 300)
PRECISIONS = (N.PRECISION_DEFAULT, N.PRECISION_FP32, N.PRECISION_BF16, N.PRECISION_X3)
ACTS = (N.ACT_RELU, N.ACT_TANH, N.ACT_ELU)
NO_RES = tuple(a | n for a in ACTS for n in (0, N.ACT_NORM))   # every activation code, with and without ACT_NORM


def test_rollout_workspaces_of_the_act_forms_equal_the_plain_ones_without_act_res():
    L = N.lib()
    for dims, n, code in itertools.product(DIMS, ROWS, NO_RES):
        d, nl = N.dims_array(dims), len(dims) - 1
        assert L.rlppo_forward_workspace_bytes_act(d, nl, n, code) == L.rlppo_forward_workspace_bytes(d, nl, n) > 0, (dims, n, code)
        assert L.rlppo_discrete_step_workspace_bytes_act(d, nl, n, code) == L.rlppo_discrete_step_workspace_bytes(d, nl, n) > 0, (dims, n, code)


def test_minibatch_workspaces_of_the_wide_forms_equal_the_narrow_ones_without_their_bits():
    L = N.lib()
    for pol, val in itertools.product(DIMS, DIMS):
        p, v = N.dims_array(pol), N.dims_array(val)
        nets = (p, len(pol) - 1, v, len(val) - 1)
        for mb, prec, critic_rows in itertools.product(ROWS, PRECISIONS, (0, 1)):
            narrow = (L.rlppo_minibatch_workspace_bytes_critic if critic_rows else L.rlppo_minibatch_workspace_bytes_for)(*nets, mb, prec)
            assert narrow > 0
            for pc, vc in itertools.product(NO_RES, NO_RES):
                case = (pol, val, mb, prec, critic_rows, pc, vc)
                normed = L.rlppo_minibatch_workspace_bytes_norm(*nets, mb, prec, critic_rows, pc, vc)
                assert L.rlppo_minibatch_workspace_bytes_res(*nets, mb, prec, critic_rows, pc, vc) == normed > 0, case
                if not (pc | vc) & N.ACT_NORM:
                    assert normed == narrow, case
