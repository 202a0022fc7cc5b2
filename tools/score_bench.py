"""Scoring given tokens: ergm_lm_score against the materialised head, and ContinuousGenerator.score end to end
(recorded in DESIGN.md 12.7, not gated by any test).

``op``: GPT-2-small head shapes (K = 768, V = 50,257, W padded to 50,304 rows; random bf16 rows of unit variance, W
scaled so that logits have a standard deviation near 3), R = 64, 512, 2048 rows, two ways on the same rows:
  fused         ops.lm_score: no logits, a workspace of (3·99 + 1)·R·4 bytes
  materialised  ops.gemm into f32 logits [R, 50304], then torch.log_softmax over the first V columns, gather of the
                target column and argmax: what a user had before (the reference of the comparison)
Call times with HIP events around the whole call, the two ways alternating inside every repeat, 1 warm-up and the
median of 5; achieved FLOP/s = 2·R·V·K over the fused call's median; the bytes each way holds at that R (logits +
log-softmax copy against the workspace).  For kernel times run one R under the profiler, in a run of its own:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/score_bench.py --case op --rows 2048
and read lm_score_kernel + lm_score_combine_kernel against the GEMM and the softmax / gather / argmax kernels.

``e2e``: GPT-2-small (random weights), 256 sequences of 64 + 64 tokens, every token from the
second on scored (128 caption tokens: the training forward takes captions of the text's length):
  native   ContinuousGenerator(max_batch=32, engine="native").score: groups of 16 sequences (2,048 packed rows)
  python   the same on engine "python": per-sequence kernels, f32 logits of a group's rows, torch.log_softmax
  forward  the parent commit's only alternative: the model's training-mode forward in eval() with labels on the same
           sequences in padded batches of 16 (bf16 logits [16·128, 50304] and one loss per batch, no per-token value)
The three alternate inside every repeat; 1 warm-up, median of 5, sequences per second over the whole call.
Without --case both run in turn, each in a fresh child process under its own timeout.
Usage (GPU box): python tools/score_bench.py [--case op|e2e] [--rows R]"""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CASES = {"op": 300, "e2e": 420}   # seconds a child may take
K, V, VPAD = 768, 50257, 50304
ROWS = (64, 512, 2048)
N_SEQ, PROMPT, REPLY, CAPS, SP1, SP2 = 256, 64, 64, 128, 50258, 50259
REPEATS = 5


def _event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _alternate(ways):
    """{name: fn} -> {name: [ms] * REPEATS}, the ways alternating inside every repeat, after one warm-up each."""
    for fn in ways.values():
        fn()
    ms = {n: [] for n in ways}
    for _ in range(REPEATS):
        for n, fn in ways.items():
            ms[n].append(_event_ms(fn))
    return ms


def _op(rows):
    import torch
    from ergm_amd import _lib as L
    from ergm_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(VPAD, K, generator=g) * (3.0 / K ** 0.5)).to(dev, torch.bfloat16)
    for R in rows:
        x = torch.randn(R, K, generator=g).to(dev, torch.bfloat16)
        t = torch.randint(0, V, (R,), generator=g).to(dev)
        need = L.load().ergm_lm_score_workspace_size(R, V, K)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        keep = {}

        def fused():
            keep["f"] = ops.lm_score(x, w, t, V, want=("logprob", "top1"), ws=ws)

        def materialised():
            logits = ops.gemm(x, w, R, VPAD, K, L.MK, L.NK, out_dtype=torch.float32)[:, :V]
            lsm = torch.log_softmax(logits, -1)
            keep["m"] = (lsm.gather(1, t[:, None])[:, 0], logits.argmax(-1))

        ms = _alternate({"fused": fused, "materialised": materialised})
        d = (keep["f"][0] - keep["m"][0]).abs().max().item()
        same_top1 = (keep["f"][3].long() == keep["m"][1]).float().mean().item()
        fm, mm = statistics.median(ms["fused"]), statistics.median(ms["materialised"])
        print(json.dumps({"case": "op", "R": R, "V": V, "K": K, "fused_ms": round(fm, 4), "materialised_ms": round(mm, 4),
                          "fused_ms_all": [round(v, 4) for v in ms["fused"]],
                          "materialised_ms_all": [round(v, 4) for v in ms["materialised"]],
                          "fused_tflops": round(2.0 * R * V * K / fm * 1e-9, 1), "fused_ws_bytes": need,
                          "materialised_bytes": 2 * R * VPAD * 4 - R * (VPAD - V) * 4,
                          "max_abs_logprob_diff": d, "top1_agree": same_top1}), flush=True)


def _e2e():
    import torch
    from ergm_amd.config import ERGMConfig, NO_DROPOUT
    from ergm_amd.generate import ContinuousGenerator
    from ergm_amd.model import GPT2LMHeadModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = GPT2LMHeadModel(ERGMConfig(**NO_DROPOUT), device=dev)
    model.eval()
    g = torch.Generator().manual_seed(1)
    n = PROMPT + REPLY
    tt = torch.cat([torch.full((1, PROMPT), SP1), torch.full((1, REPLY), SP2)], 1).to(dev)
    seqs = [(torch.randint(0, 50000, (1, n), generator=g).to(dev), tt, torch.randint(0, 50000, (1, CAPS), generator=g).to(dev),
             None, None) for _ in range(N_SEQ)]
    gens = {e: ContinuousGenerator(model, max_batch=32, max_len=n, cap_max=CAPS, engine=e) for e in ("native", "python")}
    per = 16
    batches = []
    for i in range(0, N_SEQ, per):
        ids = torch.cat([s[0] for s in seqs[i:i + per]])
        labels = ids.clone()
        labels[:, 0] = -100
        batches.append(dict(input_ids=ids, token_type_ids=tt.expand(per, n).contiguous(), labels=labels,
                            emotion_labels=torch.zeros(per, dtype=torch.long, device=dev),
                            caption_ids=torch.cat([s[2] for s in seqs[i:i + per]])))
    keep = {}

    def forward():
        with torch.no_grad():
            keep["forward"] = [float(model(**b).loss_lm) for b in batches]

    ways = {"native": lambda: keep.__setitem__("native", gens["native"].score(seqs)),
            "python": lambda: keep.__setitem__("python", gens["python"].score(seqs)), "forward": forward}
    ms = _alternate(ways)
    nll = {e: -sum(s.sum for s in keep[e]) / (N_SEQ * (n - 1)) for e in ("native", "python")}
    out = {"case": "e2e", "sequences": N_SEQ, "tokens": n, "caption_tokens": CAPS,
           "mean_nll": {**{e: round(v, 5) for e, v in nll.items()},
                        "forward": round(sum(keep["forward"]) / len(keep["forward"]), 5)}}
    for e, v in ms.items():
        med = statistics.median(v)
        out[e] = {"ms_median": round(med, 2), "ms_all": [round(x, 2) for x in v], "sequences_per_s": round(N_SEQ / med * 1e3, 1)}
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    case = args[args.index("--case") + 1] if "--case" in args else None
    rows = (int(args[args.index("--rows") + 1]),) if "--rows" in args else ROWS
    if case == "op":
        return _op(rows)
    if case == "e2e":
        return _e2e()
    if case is not None:
        raise SystemExit(f"unknown case {case!r}: one of {sorted(CASES)}")
    for c, limit in CASES.items():   # fresh child processes, one at a time; stop at the first that fails
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", c], timeout=limit)
        if r.returncode != 0:
            raise SystemExit(f"case {c} failed with exit status {r.returncode}")


if __name__ == "__main__":
    main()
