"""The mirror maps of ppo.Symmetry restated in numpy from the description alone (no packed table).  A helper module: it holds no test."""
import numpy as np

from rlgym_ppo_amd import _native as N


def obs_symmetry(d):
    """A block swap plus scattered sign flips, involutive: columns [0, h) <-> [h, 2 h), the signs of a swapped pair equal."""
    h = d // 3
    perm = np.concatenate([np.arange(h, 2 * h), np.arange(h), np.arange(2 * h, d)])
    sign = np.where(np.arange(d) % 5 == 2, -1.0, 1.0)
    sign[:h] = sign[h:2 * h] = np.where(np.arange(h) % 7 == 3, -1.0, 1.0)
    return perm, sign


def mirror_rows(x, perm, sign, ld):
    out = np.zeros((x.shape[0], ld), np.float32)
    out[:, :perm.size] = sign.astype(np.float32) * x[:, perm]
    return out


def mirror_actions(head, desc, a, bins=None):
    if head == N.HEAD_DISCRETE:
        return np.asarray(desc)[a.astype(np.int64)].astype(np.float32)
    if head == N.HEAD_MULTIDISCRETE:
        hperm, maps = desc
        src = [a[:, hperm[h]].astype(np.int64) for h in range(len(bins))]
        return np.stack([s if maps[h] is None else np.asarray(maps[h])[s] for h, s in enumerate(src)], 1).astype(np.float32)
    aperm, asign = desc
    return np.asarray(asign, np.float32) * a[:, aperm]


def mirror_mask(head, desc, m, bins=None):
    """bool [n, S] -> the mirrored rows' valid sets, from the action map alone: an action is valid <=> its image is."""
    out = np.zeros_like(m)
    if head == N.HEAD_DISCRETE:
        out[:, np.asarray(desc)] = m
        return out
    hperm, maps = desc
    starts = np.concatenate(([0], np.cumsum(bins)[:-1]))
    for h, b in enumerate(bins):
        image = np.arange(b) if maps[h] is None else np.asarray(maps[h])
        out[:, starts[h] + image] = m[:, starts[hperm[h]]:starts[hperm[h]] + b]
    return out


def pack(bits, words):
    padded = np.zeros((bits.shape[0], 32 * words), np.uint64)
    padded[:, :bits.shape[1]] = bits
    return (padded.reshape(bits.shape[0], words, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
