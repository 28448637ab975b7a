"""The yardstick of the general multi-discrete head (MultiDiscrete(nvec) of any nvec): float64 numpy / torch restated here, because
the reference's own program cannot produce a fixture for other bins -- its bins are literals (multi_discrete_policy.py:20,
torch_functions.py:101-113).  Semantics: head h owns logits [s_h, s_h + b_h), padded with -inf to B = max b_h; the distribution is
Categorical(logits=[n, H, B]); a sample is the first arg-max over c < b_h of softmax(z_h)_c / q[(row H + h) B + c] with
q = torch.empty(n H, B).exponential_(1); log p = sum_h log_softmax(z_h)[a_h]; entropy = sum_h H(z_h)."""
import ctypes

import numpy as np
import torch

from oracle import nets, ppo

REFERENCE_BINS = (3, 3, 3, 3, 3, 2, 2, 2)
NEAR_TIE = 1e-4   # two candidates' p / q within this, relative: the margin of tests/test_gpu_heads.py::test_multidiscrete_act_at_scale


def padded_logits(logits, bins):
    """torch [n, S] -> [n, H, B] with -inf beyond every head's bins (oracle/nets.py::md_logits3 for any bins)."""
    width = max(bins)
    parts = [torch.nn.functional.pad(p, (0, width - p.shape[-1]), value=float("-inf")) for p in torch.split(logits, list(bins), dim=-1)]
    return torch.stack(parts, dim=1)


def patch_oracle(monkeypatch, bins):
    """oracle.ppo.minibatch_analytic / minibatch_autograd follow oracle.nets.MD_BINS and md_logits3: with both replaced for the
    test's duration, tests/fp64_gate.gate(L, "multidiscrete", ...) runs unmodified on any bins."""
    bins = tuple(int(b) for b in bins)
    monkeypatch.setattr(nets, "MD_BINS", bins)
    monkeypatch.setattr(nets, "md_logits3", lambda logits: padded_logits(logits, bins))


def logits64(params, obs):
    p64 = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in params]
    return ppo._fwd64(p64, np.asarray(obs, np.float64))[0][-1]


def head_log_softmax64(z, bins):
    """float64 [n, S] -> list over heads of log_softmax [n, b_h]."""
    out, s = [], 0
    for b in bins:
        zz = z[:, s:s + b]
        zz = zz - zz.max(-1, keepdims=True)
        out.append(zz - np.log(np.exp(zz).sum(-1, keepdims=True)))
        s += b
    return out


def sample64(z, bins, q):
    """float64 logits [n, S], noise q [n H, B] -> (actions [n, H], logp [n], score [n, H, B] = p / q with -inf in padded slots,
    near [n, H]: the best two candidates of that head lie within NEAR_TIE of each other)."""
    n, H, B = z.shape[0], len(bins), max(bins)
    q = np.asarray(q, np.float64).reshape(n, H, B)
    act, logp, score = np.zeros((n, H), np.int64), np.zeros(n), np.full((n, H, B), -np.inf)
    for h, ls in enumerate(head_log_softmax64(z, bins)):
        b = bins[h]
        score[:, h, :b] = np.exp(ls) / q[:, h, :b]
        act[:, h] = score[:, h, :b].argmax(-1)
        logp += ls[np.arange(n), act[:, h]]
    if B > 1:
        top = np.sort(score, -1)
        near = (top[..., -1] - top[..., -2]) <= NEAR_TIE * top[..., -1]   # (a one-bin head: -inf second, never near)
    else:
        near = np.zeros((n, H), bool)
    return act, logp, score, near


def check_sampled(act, logp, z64, bins, q, max_rows=2):
    """The checks of a sampling launch against sample64: the inputs hold at most `max_rows` near-ties (asserted from the float64
    reference alone, first); indices equal except at near-ties, on at most `max_rows` rows; log-probabilities of agreeing rows
    within 1e-5; every action below its head's bin count."""
    oact, ologp, score, near = sample64(z64, bins, q)
    assert int(near.sum()) <= max_rows, ("the inputs hold too many near-ties", int(near.sum()))
    act = np.asarray(act)
    assert act.shape == oact.shape and (act >= 0).all() and (act < np.asarray(bins)[None, :]).all()
    for r, h in np.argwhere(act != oact).tolist():
        s = score[r, h]
        assert abs(s[act[r, h]] - s[oact[r, h]]) <= NEAR_TIE * s[oact[r, h]], ("index mismatch that is not a near-tie", r, h)
    same = (act == oact).all(1)
    assert same.sum() >= len(same) - max_rows
    err = float(np.abs(np.asarray(logp, np.float64)[same] - ologp[same]).max())
    print(f"[nvec] bins {tuple(bins) if len(bins) <= 8 else (bins[0], '...', len(bins))}: {int((~same).sum())} rows differ, "
          f"{int(near.sum())} near-ties, max |logp - fp64| = {err:.2e}")
    assert err < 1e-5, err
    return oact, ologp


def nvec_array(bins):
    return (ctypes.c_int32 * len(bins))(*[int(b) for b in bins])


def check_output_gradient(dz, grad_policy, S):
    """dz is the loss kernel's in-place output: its column sums over the S logits are the head layer's bias gradient (so this IS the
    buffer), and every padded column >= S is exactly zero (not the NaN the workspace was prefilled with)."""
    db = np.asarray(grad_policy[-1][1], np.float64)
    col = dz[:, :S].astype(np.float64).sum(0)
    assert np.abs(col - db).max() <= 1e-4 * max(np.abs(db).max(), 1e-30), "not the output gradient's buffer"
    assert dz.shape[1] >= S and (dz[:, S:] == 0).all() and np.isfinite(dz).all()
