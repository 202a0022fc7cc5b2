"""ergm_attn_decode per element against fp64 (tests/_decode_attn.py) at split and slot edges, through the C-ABI.

How a case runs (built once on the CPU from a seeded generator, independent data per (b, h), operands rounded to bf16):
* one launch holds a whole group of sequence lengths; it runs read-only (append = 0) and appending (append = 1), in the
  interleaved K | V layout and with K and V in separate buffers with padded rows, at every split count of the group;
* the caches are views into guard | B sequences | guard allocations filled with a sentinel outside the filled rows,
  qkv and out are views of buffers with 8 padding columns, the workspace is longer than the call may use; the pristine
  image is restored on the device before every launch;
* every element of out is compared with the fp64 reference under the derived bound, the caches bitwise with the
  expected image (appended row stored at row n_b, nothing else moved), lens, the padding and the workspace past
  B*H*splits*66 floats with what they held, and a second launch from the same image must give the same bits.
"""
import pytest
import torch

import _decode_attn as D
from ergm_amd import _lib as L
from ergm_amd import ops

pytestmark = pytest.mark.gpu

WS_SENT = -12288.0   # exact in f32; the workspace's fill
WS_SLACK = 64        # floats past the larger of what the call uses and what the size query covers
WORST = D.WORST      # (family, group) -> worst err/bound this session saw
PARAMS = [x + (lay,) for x in D.CASES for lay in D.LAYOUTS]


def _bits(t):
    return t.view(torch.int16)


def _launch(c, im, dev, splits):
    """One ergm_attn_decode call from the pristine image.  Returns the bf16 out buffer [B, E + 8] (device) after all
    the checks that do not need the reference."""
    B, E, H = c.B, c.E, c.H
    what = f"{c.name} {dev['layout']} splits {splits}"
    for d, p in zip(dev["bufs"], dev["pristine"]):
        d.copy_(p)
    eff = splits or D.auto_splits(B, H, c.max_len)
    used = B * H * eff * D.PART if eff > 1 else 0
    covered = L.load().ergm_attn_decode_workspace_size(B, H, c.max_len) // 4
    if splits == 0:
        assert used <= covered, f"{what}: the size query covers {covered} floats, the automatic choice uses {used}"
    ws = torch.full((max(used, covered) + WS_SLACK,), WS_SENT, dtype=torch.float32, device=dev["gpu"])
    out = torch.full((B, im.ldo), D.SENT, dtype=torch.bfloat16, device=dev["gpu"])
    kv = [dev["bufs"][i].as_strided((B, c.max_len, E), (im.ld_seq, im.ld_row, 1), off)
          for i, off in (im.at["k"], im.at["v"])]
    ops.attn_decode(dev["qkv"][:, :3 * E], kv[0], kv[1], dev["lens"], c.append, splits=splits, out=out[:, :E], ws=ws)
    torch.cuda.synchronize()
    assert dev["lens"].cpu().tolist() == list(c.lens), f"{what}: lens modified"
    assert torch.equal(_bits(dev["qkv"]), _bits(dev["qkv0"])), f"{what}: qkv modified"
    for i, (d, w) in enumerate(zip(dev["bufs"], dev["want"])):
        assert torch.equal(_bits(d), _bits(w)), f"{what}: cache buffer {i} is not the expected image"
    assert bool((out[:, E:] == D.SENT).all().item()), f"{what}: wrote to the padding columns of out"
    assert bool((ws[used:] == WS_SENT).all().item()), f"{what}: wrote to the workspace past {used} floats"
    assert not torch.isnan(ws[:used]).any().item(), f"{what}: NaN in a partial"
    return out


@pytest.mark.parametrize("group,family,append,layout", PARAMS, ids=[f"{D.case_id(*x[:3])}-{x[3]}" for x in PARAMS])
def test_decode_attn(gpu, group, family, append, layout):
    """Every element within the bound of the fp64 reference at every split count of the case; caches, lens, padding and
    workspace as they must be; a second run bitwise the same; rows with n_b = 0 exact."""
    c = D.group_case(group, family, append)
    im = D.image(c, layout)
    dev = dict(gpu=gpu, layout=layout, bufs=[b.to(gpu) for b in im.bufs], pristine=[b.to(gpu) for b in im.bufs],
               want=[b.to(gpu) for b in im.want], qkv=im.qkv.to(gpu), qkv0=im.qkv.to(gpu),
               lens=torch.tensor(c.lens, dtype=torch.int32, device=gpu))
    E = c.E
    for splits in D.case_splits(group, family):
        what = f"{D.case_id(group, family, append)} {layout} splits {splits}"
        out = _launch(c, im, dev, splits)
        again = _launch(c, im, dev, splits)
        assert torch.equal(_bits(out), _bits(again)), f"{what}: not bitwise repeatable"
        got = out[:, :E].cpu()
        worst = D.check(c, what, got)
        print(f"{what}: worst err/bound {worst:.4f}")
        for b, nb in enumerate(c.n):
            if nb == 0:   # append = 0: a zero row; append = 1: attention over the new row alone = the new V
                exp = c.qkv[b, 2 * E:] if append else torch.zeros(E, dtype=torch.bfloat16)
                assert torch.equal(_bits(got[b]), _bits(exp)), f"{what}: sequence {b} (n = 0) is not exact"


def test_worst_ratios(gpu):
    """Prints the worst err/bound per family and group that this session's tests saw."""
    D.report()
