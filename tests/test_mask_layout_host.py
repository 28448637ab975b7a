"""util.action_mask.Layout, the one owner of mask geometry and mask rules, without a GPU: the reference-sized multi-discrete layout
(bins 2, 7, 3, 11, 2 -- 25 logits in one word) and a discrete layout of 33 actions, which crosses a word boundary.  The packed
encoding is restated bit by bit; the per-head rule and the all-valid fallback are restated with plain loops over the heads."""
import numpy as np
import pytest
import torch

BINS = (2, 7, 3, 11, 2)
S = sum(BINS)
STARTS = [0, 2, 9, 12, 23]
A = 33


def layouts():
    from rlgym_ppo_amd.util.action_mask import Layout
    return Layout(S, BINS), Layout(A)


def segments(lay):
    """[(start, stop)] of every head; the discrete head is one head."""
    return [(0, lay.width)] if lay.heads is None else [(s, s + b) for s, b in zip(STARTS, BINS)]


def rand_mask(lay, n, seed):
    """bool [n, width]: every head of every row keeps a valid bin; row 1 all valid, row 2 exactly one valid bin per head (the last)."""
    rs = np.random.RandomState(seed)
    m = rs.rand(n, lay.width) < 0.5
    for lo, hi in segments(lay):
        m[np.arange(n), rs.randint(lo, hi, n)] = True
    m[1] = True
    m[2] = False
    m[2, [hi - 1 for _, hi in segments(lay)]] = True
    return m


def restate(mask):
    """The encoding, bit by bit: bit c % 32 of word c / 32 = entry c."""
    n, width = mask.shape
    out = np.zeros((n, (width + 31) // 32), np.uint64)
    for r in range(n):
        for c in range(width):
            if mask[r, c]:
                out[r, c // 32] |= np.uint64(1) << np.uint64(c % 32)
    return out.astype(np.uint32)


def test_fields_and_immutability():
    md, flat = layouts()
    assert (md.width, md.heads, md.words, list(md.starts)) == (S, BINS, 1, STARTS)
    assert (flat.width, flat.heads, flat.words, list(flat.starts)) == (A, None, 2, [0])
    with pytest.raises(AttributeError):
        md.width = 26
    with pytest.raises(ValueError):
        md.starts[1] = 3
    from rlgym_ppo_amd.util.action_mask import Layout
    for width, heads in ((S + 1, BINS), (S, BINS[:-1]), (2, (2, 0)), (0, ())):
        with pytest.raises(ValueError, match="layout"):
            Layout(width, heads)
    with pytest.raises(ValueError, match="layout"):
        Layout(0)


@pytest.mark.parametrize("which", [0, 1])
def test_pack_host_is_the_encoding_and_unpack_inverts_it(which):
    lay = layouts()[which]
    m = rand_mask(lay, 19, 3 + which)
    words = lay.pack_host(m)
    assert words.dtype == np.int32 and words.shape == (19, lay.words) and np.array_equal(words.view(np.uint32), restate(m))
    if lay.width % 32:   # bits at and beyond the width are clear
        assert (words.view(np.uint32)[:, -1] >> np.uint32(lay.width % 32)).max() == 0
    back = lay.unpack(torch.from_numpy(words))
    assert back.dtype == torch.bool and np.array_equal(back.numpy(), m)
    for form in (m.astype(np.float32), m.astype(np.int64), m.tolist(), torch.from_numpy(m)):
        got = lay.pack(form, "cpu")
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), words)


@pytest.mark.parametrize("which", [0, 1])
def test_a_rank_1_mask_is_one_row_and_a_wrong_width_raises(which):
    lay = layouts()[which]
    m = rand_mask(lay, 4, 11)
    assert lay.rows(m[3]).shape == (1, lay.width) and np.array_equal(lay.rows(m[3])[0], m[3])
    assert np.array_equal(lay.pack_host(m[3]), lay.pack_host(m)[3:4])
    assert np.array_equal(lay.valid(m[3], "cpu").numpy(), m[3:4])
    assert lay.rows(m.astype(np.float32)).dtype == bool
    for bad in (np.ones((4, lay.width + 1), bool), np.ones(lay.width - 1, bool), np.ones((2, 2, lay.width), bool)):
        with pytest.raises(ValueError, match="shape"):
            lay.rows(bad)
        with pytest.raises(ValueError, match="shape"):
            lay.pack_host(bad)


def test_first_empty_is_the_first_row_then_its_first_head():
    md, flat = layouts()
    m = rand_mask(md, 9, 5)
    one = np.zeros((9, S), bool)
    one[:, [s + b - 1 for s, b in zip(STARTS, BINS)]] = True      # exactly one valid bin in every head of every row
    assert md.first_empty(m) is None and md.first_empty(one) is None and md.first_empty(one[:0]) is None
    m[6, 12:23] = False                                           # row 6: head 3
    m[4, 23:25] = False                                           # row 4: head 4 ...
    m[4, 2:9] = False                                             # ... and head 1: the first row, then its first head
    assert md.first_empty(m) == (4, 1)
    with pytest.raises(ValueError, match=r"action mask: row 4, head 1 \(bins 2 \.\. 8\) has no valid bin"):
        md.pack_host(m)
    m[4, 5] = True
    assert md.first_empty(m) == (4, 4) and md.what(4) == ", head 4 (bins 23 .. 24) has no valid bin"
    m[4, 24] = True
    assert md.first_empty(m) == (6, 3)
    f = rand_mask(flat, 9, 6)
    one = np.zeros((9, A), bool)
    one[:, 32] = True                                             # the one valid action sits in the second word
    assert flat.first_empty(f) is None and flat.first_empty(one) is None
    f[7] = False
    f[3] = False
    assert flat.first_empty(f) == (3, None) and flat.what(None) == " has no valid action"
    with pytest.raises(ValueError, match="action mask: row 3 has no valid action"):
        flat.pack_host(f)


@pytest.mark.parametrize("which", [0, 1])
def test_valid_applies_the_all_valid_fallback_per_head(which):
    from rlgym_ppo_amd.util.action_mask import Packed
    lay = layouts()[which]
    m = rand_mask(lay, 8, 7)
    segs = segments(lay)
    lo, hi = segs[len(segs) // 2]
    m[5, lo:hi] = False                                           # one head of row 5 without a valid bin
    m[6] = False                                                  # every head of row 6
    want = m.copy()
    for r in range(8):
        for a, b in segs:
            if not m[r, a:b].any():
                want[r, a:b] = True
    assert not np.array_equal(want, m) and want[6].all() and np.array_equal(want[:5], m[:5])
    # a tensor or packed words may hold such a head (they stand for device masks, which are never read back) ...
    got = lay.valid(torch.from_numpy(m), "cpu")
    assert got.dtype == torch.bool and tuple(got.shape) == (8, lay.width) and np.array_equal(got.numpy(), want)
    words = torch.from_numpy(restate(m).view(np.int32))           # (the words of m itself: pack_host would refuse it)
    assert np.array_equal(lay.valid(Packed(words, lay.width), "cpu").numpy(), want)
    with pytest.raises(ValueError, match="packed action mask"):
        lay.valid(Packed(words, lay.width + 1), "cpu")
    # ... a host array is held to the rule, and passes through unchanged when it keeps it
    with pytest.raises(ValueError, match="row 5"):
        lay.valid(m, "cpu")
    assert np.array_equal(lay.valid(want, "cpu").numpy(), want)


def test_layout_of_a_policy():
    from rlgym_ppo_amd.util.action_mask import Layout

    class Own:
        mask_layout = Layout(S, BINS)
        n_actions = 4            # (ignored: the policy states its layout)

    class Duck:
        n_logits, splits = S, list(BINS)

    class DiscreteLike:
        mask_layout = None       # (ArenaModule's default)
        n_actions = A

    class Neither:
        mask_layout = None

    own = Own()
    assert Layout.of(own) is own.mask_layout
    duck = Layout.of(Duck())
    assert (duck.width, duck.heads, duck.words, list(duck.starts)) == (S, BINS, 1, STARTS)
    flat = Layout.of(DiscreteLike())
    assert (flat.width, flat.heads, flat.words) == (A, None, 2)
    from rlgym_ppo_amd.util import action_mask as AM
    with pytest.raises(ValueError) as e:
        Layout.of(Neither())
    assert str(e.value).startswith(AM.REFUSAL + ", not of Neither")
    assert "option of the discrete head (DiscreteFF) and of the multi-discrete head (MultiDiscreteFF)" in AM.REFUSAL


def test_the_module_functions_give_the_layouts_results():
    from rlgym_ppo_amd.util import action_mask as AM
    md, flat = layouts()
    m, f = rand_mask(md, 12, 8), rand_mask(flat, 12, 9)
    assert AM.mask_words(S) == md.words and AM.mask_words(A) == flat.words
    assert np.array_equal(AM.pack_host(m, S, heads=BINS), md.pack_host(m)) and np.array_equal(AM.pack_host(m, S, heads=list(BINS)), md.pack_host(m))
    assert np.array_equal(AM.pack_host(f, A), flat.pack_host(f))
    assert torch.equal(AM.pack(m, S, "cpu", heads=BINS), md.pack(m, "cpu")) and torch.equal(AM.pack(f, A, "cpu"), flat.pack(f, "cpu"))
    assert torch.equal(AM.unpack(flat.pack(f, "cpu"), A), flat.unpack(flat.pack(f, "cpu")))
    packed = AM.Packed(flat.pack(f, "cpu"), A)
    assert packed.shape == (12, A) and np.array_equal(packed.unpack().numpy(), f) and flat.pack(packed, "cpu") is not None
    AM.check_heads(m, BINS)
    m[9, 9:12] = False
    for call in (lambda: AM.check_heads(m, BINS), lambda: AM.pack_host(m, S, heads=BINS), lambda: md.checked(m)):
        with pytest.raises(ValueError, match=r"action mask: row 9, head 2 \(bins 9 \.\. 11\) has no valid bin"):
            call()
    assert np.array_equal(AM.pack_host(m, S), AM.Layout(S).pack_host(m))   # without heads: the row keeps a valid action
