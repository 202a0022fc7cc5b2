"""In-step A/B of the row-count LM-head dX plan: (cfg, split, one-K-slice-per-XCD) variants through
ergm_gemm_set_override / ERGM_DYN_XCD inside the running bench step (as tools/step_tune.py measures).
usage: python tools/lmhead_rows_tune.py --config c2|c4|c5 [--rounds 3]   (profiles/r07_lmhead_rows_plan_ab.txt)"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ergm_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c2")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=30)
args = ap.parse_args()
from ergm_amd.config import ERGMConfig  # noqa: E402
from ergm_amd.data import synthetic_batch  # noqa: E402
from ergm_amd.model import GPT2LMHeadModel  # noqa: E402
from ergm_amd.optim import FusedAdamW  # noqa: E402

dev = torch.device("cuda:0")
mname, S, turns, B, Fd, fp8, _ = bench.CONFIGS[args.config]
cfg = ERGMConfig(**bench.MODELS[mname], feat_dim=Fd, fp8=fp8)
model = GPT2LMHeadModel(cfg, device=dev)
model.init_weights(seed=0)
opt = FusedAdamW([model.flat], lr=2e-5, model=model, overlap=True)
batch = synthetic_batch(B, S, n_turns=turns, seed=1000, feat_dim=Fd)
kw = dict(input_ids=batch["input_ids"], token_type_ids=batch["token_type_ids"], labels=batch["labels"],
          emotion_labels=batch["emotion_labels"], caption_ids=batch["caption_ids"], imgs=batch["visual_feat"],
          auds=batch["audio_feat"])
kw = {k: v.to(dev) for k, v in kw.items()}
lib = L.load()
T, E, Vp = B * S, cfg.n_embd, model.layout.vocab_pad


def step():
    out = model(**kw)
    opt.zero_grad()
    out.loss.backward()
    opt.step()


def measure(steps=args.steps):
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / steps


def set_variant(v):
    c, sp, xcd = v
    L.check(lib.ergm_gemm_set_override(T, E, Vp, L.MK, L.KN, c, sp), "override")
    os.environ["ERGM_DYN_XCD"] = str(xcd)


variants = [(c, sp, x) for c in (14, 2) for sp in (16, 8) for x in (1, 0)] + [(0, 16, 1), (0, 8, 1)]
for _ in range(10):
    step()
tot = {v: 0.0 for v in variants}
for r in range(args.rounds):
    for v in variants:
        set_variant(v)
        tot[v] += measure()
print(f"{args.config}: T={T} E={E} Vp={Vp}; ms/step mean of {args.rounds} interleaved rounds of {args.steps} steps")
for v in sorted(variants, key=lambda v: tot[v]):
    print(f"  cfg {v[0]:2d} split {v[1]:2d} xcd {v[2]}: {tot[v] / args.rounds:.3f}")
