"""The launches of the logit rules alone, for a kernel trace: B = 32 rows of GPT-2's vocabulary with
histories of ``--len`` tokens (128 or 1024) over a small alphabet, so the n-gram rule (n = 3) finds matches at many
positions, 8 one-token bad words per row, and the three history kernels beside it.  Per-launch times come from
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/rules_bench.py --len 128
(one run per length; the kernels' names are the same).  Without a profiler it prints event-timed means, which include
the launch gaps of a back-to-back stream and are an upper bound only.
Usage (GPU box): python tools/rules_bench.py [--len L] [--iters N]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import torch
    from ergm_amd import ops
    arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
    L_, iters = arg("--len", 128), arg("--iters", 200)
    B, V, ldl, W, max_len, eos = 32, 50257, 50304, 4, 1024, 50256
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, ldl, generator=g).to(dev)
    hist = torch.randint(0, 5, (B, max_len), generator=g, dtype=torch.int32).to(dev)
    lens = torch.full((B,), L_ - 1, dtype=torch.int32, device=dev)   # the append lands at L - 1: inside the cache
    start = torch.zeros(B, dtype=torch.int32, device=dev)
    ngram = torch.full((B,), 3, dtype=torch.int32, device=dev)
    bad = torch.tensor([[1, 1000 * i + 7] for i in range(1, 9)], dtype=torch.int32).reshape(1, -1).repeat(B, 1)
    bad = torch.cat([bad, torch.zeros(B, 64 - bad.shape[1], dtype=torch.int32)], 1).to(dev)
    fin = torch.zeros(B, dtype=torch.uint8, device=dev)
    tokens = torch.randint(0, 5, (B,), generator=g).to(dev)
    parent = torch.tensor([r - r % W for r in range(B)], dtype=torch.int32, device=dev)   # W - 1 of W rows move
    ids = torch.randint(0, 5, (B * L_,), generator=g).to(dev)
    slot = torch.arange(B, dtype=torch.int32, device=dev)
    q0 = slot * L_
    n = torch.full((B,), L_, dtype=torch.int32, device=dev)
    rules = ops.rules_desc(hist, start=start, ngram=ngram, bad=bad)
    fns = {"logit_rules_apply": lambda: ops.logit_rules(logits, V, rules, lens, eos, max_len, finished=fin),
           "hist_append": lambda: ops.hist_append(tokens, lens, hist, max_len, finished=fin),
           "hist_follow": lambda: ops.hist_follow(hist, parent, lens, W, max_len),
           "hist_write": lambda: ops.hist_write(ids, slot, q0, n, hist, max_len)}
    out = {"B": B, "V": V, "history": L_, "iters": iters}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name + "_us_back_to_back"] = round(e0.elapsed_time(e1) * 1e3 / iters, 2)
    out["banned_per_row_mean"] = round(float(torch.isinf(logits[:, :V]).sum().item()) / B, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
