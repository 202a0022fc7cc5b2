"""ergm_beam_seed alone: behind an admission that filled row g·W of a group, the caption rows [0, c) of every layer reach
the group's other slots and nothing else is written; the per-row state takes the stated values; a caption length on the
device above cap_max or below 0 clamps; a group id on the device outside [0, G) writes nothing.  Caches are filled
with a sentinel, so every comparison is of whole tensors, bitwise."""
import math

import pytest
import torch

from ergm_amd import ops

pytestmark = pytest.mark.gpu
SENT = 0x5A5A
G = 4
# (layers, row width in int16, cap_max): rows of 1,280 bytes (a lane takes two pieces); 50 layers of one 16-byte piece
# per row (two launches: 48 + 2); 70 caption rows (two 64-row chunks)
SHAPES = [(2, 640, 16), (50, 8, 16), (2, 8, 70)]


def _state(mb, gpu):
    r = torch.arange(mb, dtype=torch.int32)
    return dict(lens=(77 + r).to(gpu), cap_lens=(55 + r).to(gpu), stop_lens=(99 + r).to(gpu),
                finished=torch.full((mb,), 9, dtype=torch.uint8, device=gpu), scores=(5.0 + r.float()).to(gpu))


def _seed_case(gpu, W, n_layer, width, cap_max, groups, caps, dev_caps=None, groups_dev=None):
    """Fill, seed, and return (before, after, state before, state after, the caption length each group's row holds)."""
    mb, rows = G * W, cap_max + 3
    g = torch.Generator().manual_seed(5 + W + n_layer)
    xkv = [torch.full((mb, rows, width), SENT, dtype=torch.int16, device=gpu) for _ in range(n_layer)]
    st = _state(mb, gpu)
    held = {}
    for grp, c in zip(groups, caps):
        r0 = grp * W
        for t in xkv:   # the admission's rows; what lies behind them in the slot stays sentinel
            t[r0, :c] = torch.randint(0, 1000, (c, width), generator=g, dtype=torch.int16).to(gpu)
        held[grp] = c if dev_caps is None else dev_caps[grp]
        st["lens"][r0], st["cap_lens"][r0], st["stop_lens"][r0], st["finished"][r0] = 5 + grp, held[grp], 20 + grp, 0
    before = [t.clone() for t in xkv]
    st0 = {k: v.clone() for k, v in st.items()}
    ops.beam_seed(xkv, groups, W, cap_max, st["lens"], st["cap_lens"], st["stop_lens"], st["finished"], st["scores"],
                  groups_dev=groups_dev)
    torch.cuda.synchronize()
    return before, xkv, st0, st, held


def _expect(before, st0, W, cap_max, seeded, held):
    caches = [t.clone() for t in before]
    st = {k: v.clone() for k, v in st0.items()}
    for grp in seeded:
        r0, c = grp * W, max(0, min(held[grp], cap_max))
        st["scores"][r0] = 0.0
        for w in range(1, W):
            for t, b in zip(caches, before):
                t[r0 + w, :c] = b[r0, :c]
            st["lens"][r0 + w], st["cap_lens"][r0 + w], st["stop_lens"][r0 + w] = 0, c, st0["stop_lens"][r0]
            st["finished"][r0 + w], st["scores"][r0 + w] = 0, -math.inf
    return caches, st


def _same(got_caches, got_st, want_caches, want_st):
    for l, (a, b) in enumerate(zip(got_caches, want_caches)):
        assert torch.equal(a, b), f"layer {l}"
    for k in want_st:
        a, b = got_st[k], want_st[k]
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k


@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("n_layer,width,cap_max", SHAPES)
def test_seed_copies_the_captions_and_sets_the_rows(gpu, W, n_layer, width, cap_max):
    """Groups (3, 0, 2) of 4, out of order and with the last one, caption lengths 1, 7 and cap_max; group 1 is not named
    and stays as it was, every row of it."""
    groups, caps = (3, 0, 2), (1, 7, cap_max)
    before, after, st0, st, held = _seed_case(gpu, W, n_layer, width, cap_max, groups, caps)
    want_c, want_s = _expect(before, st0, W, cap_max, groups, held)
    _same(after, st, want_c, want_s)
    if W > 1:   # the copy happened: a destination holds its source's rows and the sentinel behind them
        assert torch.equal(after[-1][2 * W + W - 1, :cap_max], before[-1][2 * W, :cap_max])
        assert int((after[0][1] != SENT).sum()) == 7 * width and int((after[0][W:2 * W] != SENT).sum()) == 0
        assert st["scores"][:W].tolist() == [0.0] + [-math.inf] * (W - 1)
        assert st["cap_lens"][3 * W:].tolist() == [1] * W and st["lens"][3 * W:].tolist() == [5 + 3] + [0] * (W - 1)
    else:
        assert all(torch.equal(a, b) for a, b in zip(after, before))
    assert st["lens"][W:2 * W].tolist() == st0["lens"][W:2 * W].tolist()   # the idle group


@pytest.mark.parametrize("n_layer,width,cap_max", SHAPES[:2])
def test_a_caption_length_outside_the_cache_clamps(gpu, n_layer, width, cap_max):
    """cap_lens[g·W] = cap_max + 5 and -3 on the device: cap_max rows and no row are copied, the rows behind cap_max keep
    the sentinel, the group's other rows get the clamped value, and row g·W keeps what it held."""
    W, groups = 2, (1, 3)
    dev_caps = {1: cap_max + 5, 3: -3}
    before, after, st0, st, held = _seed_case(gpu, W, n_layer, width, cap_max, groups, (cap_max, 4), dev_caps=dev_caps)
    want_c, want_s = _expect(before, st0, W, cap_max, groups, held)
    _same(after, st, want_c, want_s)
    assert st["cap_lens"].tolist()[2:4] == [cap_max + 5, cap_max] and st["cap_lens"].tolist()[6:8] == [-3, 0]
    for t in after:
        assert int((t[:, cap_max:] != SENT).sum()) == 0 and int((t[7] != SENT).sum()) == 0


def test_a_group_id_outside_the_range_writes_nothing(gpu):
    """The kernels read the ids from the device array: (3, 4, -1) there seeds group 3 alone."""
    W, cap_max = 4, 16
    groups_dev = torch.tensor([3, G, -1], dtype=torch.int32, device=gpu)
    before, after, st0, st, held = _seed_case(gpu, W, 2, 640, cap_max, (3, 0, 2), (5, 7, 9), groups_dev=groups_dev)
    want_c, want_s = _expect(before, st0, W, cap_max, (3,), held)
    _same(after, st, want_c, want_s)
    assert st["scores"][0].item() == 5.0 and st["scores"][3 * W].item() == 0.0


def test_refusals_launch_nothing(gpu):
    W, cap_max = 2, 16
    for bad in ((0, 4), (1, 1), (-1,), ()):
        mb = G * W
        xkv = [torch.full((mb, cap_max, 8), SENT, dtype=torch.int16, device=gpu) for _ in range(2)]
        st = _state(mb, gpu)
        st0 = {k: v.clone() for k, v in st.items()}
        with pytest.raises(ValueError):
            ops.beam_seed(xkv, bad, W, cap_max, st["lens"], st["cap_lens"], st["stop_lens"], st["finished"], st["scores"])
        torch.cuda.synchronize()
        _same(xkv, st, [torch.full_like(t, SENT) for t in xkv], st0)
    with pytest.raises(ValueError):
        ops.beam_seed(xkv, (0,), 3, cap_max, st["lens"], st["cap_lens"], st["stop_lens"], st["finished"], st["scores"])
    with pytest.raises(ValueError):
        ops.beam_seed([t[:, :, :4] for t in xkv], (0,), W, cap_max, st["lens"], st["cap_lens"], st["stop_lens"], st["finished"],
                      st["scores"])
