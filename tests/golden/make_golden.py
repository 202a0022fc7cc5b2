"""Generate the golden fixtures that pin ``oracle/gpt2_oracle.py`` to the reference.

Runs ONLY in the build container (needs ``/root/reference``).  It imports the reference model
(``/root/reference/src/model.py``) through the loader shim of SURVEY.md §8(c) — no source edits,
bytecode writing disabled — loads seeded weights with ``load_state_dict(strict=True)``, runs the
training-mode forward + backward exactly as the only runnable reference call does (with
``caption_ids``), checks the oracle restatement against it, and writes the reference's own outputs
as ``tests/golden/*.npz``.  Also pins the AdamW / LR-schedule restatement against
``torch.optim.AdamW`` + ``transformers.get_polynomial_decay_schedule_with_warmup`` (the third-party
code src/main.py:68,93-95 calls).

Also captures, from the reference's own code: the 2-D ``imgs`` semantics (src/model.py:497), the
data pipeline (``CustomDataset`` + ``PadCollate``, src/custom_dataset.py) on synthetic pickles, and
three steps of the src/main.py training loop with its reported metrics.

Usage:  python tests/golden/make_golden.py [--only imgs2d,dataset,trainer]
"""
from __future__ import annotations

import json
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import gpt2_oracle as O  # noqa: E402
from ergm_amd.data import synthetic_batch  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from _golden import save_npz  # noqa: E402

REF_SRC = "/root/reference/src"


def load_reference():
    """Loader shim: stub 4 names removed from transformers 5.x, 4.26 get_head_mask
    semantics, map the hard-coded ``.to("cuda")`` (src/model.py:401-408) to CPU, dict tied keys."""
    import torch.nn as nn
    import transformers.modeling_utils as mu
    import transformers.pytorch_utils as pu
    if not hasattr(mu, "SequenceSummary"):
        mu.SequenceSummary = object
    for n in ("find_pruneable_heads_and_indices", "prune_conv1d_layer"):
        if not hasattr(pu, n):
            setattr(pu, n, lambda *a, **k: None)
    m = types.ModuleType("transformers.utils.model_parallel_utils")
    m.assert_device_map = lambda *a, **k: None
    m.get_device_map = lambda *a, **k: None
    sys.modules["transformers.utils.model_parallel_utils"] = m
    mu.PreTrainedModel.get_head_mask = lambda self, hm, n, *a, **k: [None] * n
    if not getattr(nn.Module.to, "_ergm_shim", False):
        _to = nn.Module.to

        def _to_cpu(self, *a, **k):
            a = tuple("cpu" if isinstance(x, str) and x.startswith("cuda") else x for x in a)
            return _to(self, *a, **k)
        _to_cpu._ergm_shim = True
        nn.Module.to = _to_cpu
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import model as refmodel  # the reference's src/model.py
    refmodel.GPT2LMHeadModel._tied_weights_keys = {"lm_head.weight": "transformer.wte.weight"}
    return refmodel


def ref_run(refmodel, cfg: O.OracleConfig, P, batch):
    from transformers import GPT2Config
    gcfg = GPT2Config(vocab_size=cfg.vocab_size, n_embd=cfg.n_embd, n_layer=cfg.n_layer,
                      n_head=cfg.n_head, n_positions=cfg.n_positions, n_inner=cfg.n_inner,
                      attn_pdrop=0.0, resid_pdrop=0.0, embd_pdrop=0.0,
                      layer_norm_epsilon=cfg.layer_norm_epsilon)
    net = refmodel.GPT2LMHeadModel(gcfg)
    sd = dict(P)
    sd["lm_head.weight"] = P["transformer.wte.weight"]
    net.load_state_dict(sd, strict=True)
    assert net.lm_head.weight.data_ptr() == net.transformer.wte.weight.data_ptr(), "lm_head not tied"
    net.train()
    kw = dict(input_ids=batch["input_ids"], token_type_ids=batch["token_type_ids"],
              labels=batch["labels"], emotion_labels=batch["emotion_labels"],
              caption_ids=batch["caption_ids"])
    if batch.get("visual_feat") is not None:
        kw["imgs"] = batch["visual_feat"]       # [B, Tv, E]: imgs[i][0] is row 0 (src/model.py:497)
        kw["auds"] = batch["audio_feat"]        # [B, E] (src/model.py:498)
    out = net(**kw)
    out.loss.backward()
    grads = {}
    for name, p in net.named_parameters():
        grads[name] = p.grad.detach().clone()
    # lm_head is tied: its grad is folded into wte's (named_parameters yields the shared tensor once)
    return out, grads


def compare(tag, a, b, rtol):
    a, b = a.double(), b.double()
    err = (a - b).norm() / max(b.norm().item(), 1e-30)
    ok = err.item() <= rtol
    print(f"  {tag:55s} rel-L2 {err.item():.3e} {'ok' if ok else 'FAIL'}")
    return ok


def build_case(refmodel, name, cfg, B, S, seed, with_features=True, visual_rows=1, n_turns=5,
               full_grads=True, vocab_hi=None, xpeak=None):
    print(f"[{name}] L={cfg.n_layer} E={cfg.n_embd} H={cfg.n_head} V={cfg.vocab_size} B={B} S={S}"
          + (f" cross-attention gains {xpeak}" if xpeak else ""))
    P = O.init_params(cfg, seed=seed)
    if xpeak:  # peaked cross-attention (oracle.peak_cross_attention): every gradient at the model's scale
        O.peak_cross_attention(P, cfg.n_layer, *xpeak)
    vhi = vocab_hi if vocab_hi is not None else cfg.vocab_size - 3
    batch = synthetic_batch(B, S, n_turns=n_turns, feat_dim=cfg.n_embd, seed=seed + 1000,
                            vocab_hi=vhi, visual_rows=visual_rows, with_features=with_features,
                            sp1=cfg.vocab_size - 2, sp2=cfg.vocab_size - 1, eos=vhi - 1)
    ref_out, ref_g = ref_run(refmodel, cfg, P, batch)
    ora_out, ora_g = O.loss_and_grads(P, cfg, batch)
    ok = True
    ok &= compare("loss", ora_out["loss"].reshape(1), ref_out.loss.detach().reshape(1), 1e-5)
    ok &= compare("logits", ora_out["logits"], ref_out.logits.detach(), 1e-5)
    ok &= compare("emotion_logits", ora_out["emotion_logits"], ref_out.emotion_logits.detach(), 1e-5)
    for k in ora_g:
        ok &= compare("grad " + k, ora_g[k], ref_g[k], 1e-4)
    assert ok, f"oracle does not match the reference on {name}"
    rec = {
        "config": np.array([cfg.vocab_size, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_positions],
                           dtype=np.int64),
        "seed": np.array(seed),
        **({"xpeak_gains": np.array(xpeak, dtype=np.float64)} if xpeak else {}),
        "loss": ref_out.loss.detach().numpy(),
        "loss_lm": ora_out["loss_lm"].numpy(),
        "loss_emotion": ora_out["loss_emotion"].numpy(),
        "emotion_logits": ref_out.emotion_logits.detach().numpy(),
    }
    for k, v in batch.items():
        rec["in_" + k] = v.numpy()
    logits = ref_out.logits.detach()
    if logits.numel() <= 200_000:
        rec["logits"] = logits.numpy()
    else:
        rec["logits_head"] = logits[:, :4, :64].numpy().copy()
        rec["logits_tail"] = logits[:, -2:, -64:].numpy().copy()
        rec["logits_rowsum"] = logits.sum(-1).numpy()
    for k, g in ref_g.items():
        if full_grads:
            rec["grad:" + k] = g.numpy()
        else:
            rec["gradnorm:" + k] = np.array(g.double().norm().item())
            rec["gradhead:" + k] = g.reshape(-1)[:32].numpy().copy()
    return P, batch, rec


def adamw_case():
    """Two AdamW steps under the poly-decay schedule vs torch.optim.AdamW + transformers schedule."""
    from transformers import get_polynomial_decay_schedule_with_warmup
    g = torch.Generator().manual_seed(7)
    shapes = {"a": (33, 17), "b": (64,)}
    P = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    grads = [{k: torch.randn(s, generator=g) for k, s in shapes.items()} for _ in range(3)]
    lr, warm, total = 2e-5, 1, 5
    tp = {k: torch.nn.Parameter(v.clone()) for k, v in P.items()}
    opt = torch.optim.AdamW(list(tp.values()), lr=lr, foreach=False)
    sched = get_polynomial_decay_schedule_with_warmup(opt, num_warmup_steps=warm, num_training_steps=total,
                                                      power=2)
    lrs = []
    for G in grads:
        for k, p in tp.items():
            p.grad = G[k].clone()
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    st = O.AdamWState()
    mine = {k: v.clone() for k, v in P.items()}
    my_lrs = []
    for i, G in enumerate(grads):
        cur = O.poly_decay_lr(i, lr, warm, total)
        my_lrs.append(cur)
        O.adamw_step(mine, G, st, cur)
    assert np.allclose(lrs, my_lrs, rtol=1e-12, atol=0), (lrs, my_lrs)
    for k in P:
        assert torch.allclose(mine[k], tp[k].detach(), rtol=1e-6, atol=1e-9), k
    # the schedule over a longer horizon (warmup 10%, as src/main.py:91 default warmup_ratio=0.1)
    lr2, total2 = 2e-5, 40
    warm2 = int(0.1 * total2)
    opt2 = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr2)
    s2 = get_polynomial_decay_schedule_with_warmup(opt2, num_warmup_steps=warm2, num_training_steps=total2,
                                                   power=2)
    ref_lrs = []
    for _ in range(total2 + 3):
        ref_lrs.append(opt2.param_groups[0]["lr"])
        opt2.step()
        s2.step()
    print("  adamw + schedule restatement ok")
    rec = {"lrs": np.array(lrs), "sched_lrs": np.array(ref_lrs),
           "sched_args": np.array([lr2, warm2, total2])}
    for k in P:
        rec["p0:" + k] = P[k].numpy()
        rec["p3:" + k] = tp[k].detach().numpy()
        for i, G in enumerate(grads):
            rec[f"g{i}:" + k] = G[k].numpy()
    return rec


def imgs2d_case(refmodel):
    """The reference's imgs[i][0] (src/model.py:497) on a 2-D [B, E] ``imgs`` tensor: the SCALAR
    imgs[i, 0], broadcast over position 0's embedding (vs row 0 of a 3-D tensor)."""
    cfg = O.OracleConfig(vocab_size=256, n_embd=64, n_layer=2, n_head=1, n_positions=64)
    seed = 55
    print(f"[imgs2d_e64] 2-D imgs, L={cfg.n_layer} E={cfg.n_embd}")
    P = O.init_params(cfg, seed=seed)
    batch = synthetic_batch(2, 32, n_turns=3, feat_dim=cfg.n_embd, seed=seed + 1000, vocab_hi=253, sp1=254,
                            sp2=255, eos=252)
    imgs = batch.pop("visual_feat")[:, 0].contiguous()   # [B, E]
    from transformers import GPT2Config
    gcfg = GPT2Config(vocab_size=cfg.vocab_size, n_embd=cfg.n_embd, n_layer=cfg.n_layer, n_head=cfg.n_head,
                      n_positions=cfg.n_positions, attn_pdrop=0.0, resid_pdrop=0.0, embd_pdrop=0.0)
    net = refmodel.GPT2LMHeadModel(gcfg)
    sd = dict(P)
    sd["lm_head.weight"] = P["transformer.wte.weight"]
    net.load_state_dict(sd, strict=True)
    net.train()
    out = net(input_ids=batch["input_ids"], token_type_ids=batch["token_type_ids"], labels=batch["labels"],
              emotion_labels=batch["emotion_labels"], caption_ids=batch["caption_ids"], imgs=imgs,
              auds=batch["audio_feat"])
    out.loss.backward()
    ref_g = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    ora, og = O.loss_and_grads(P, cfg, dict(batch, imgs=imgs))
    ok = compare("loss", ora["loss"].reshape(1), out.loss.detach().reshape(1), 1e-5)
    ok &= compare("logits", ora["logits"], out.logits.detach(), 1e-5)
    for k in og:
        ok &= compare("grad " + k, og[k], ref_g[k], 1e-4)
    vec, _ = O.loss_and_grads(P, cfg, dict(batch, visual_feat=imgs))
    assert abs(vec["loss"].item() - out.loss.item()) > 1e-6, "2-D imgs must differ from the vector form"
    assert ok
    rec = {"config": np.array([cfg.vocab_size, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_positions]),
           "seed": np.array(seed), "loss": out.loss.detach().numpy(), "logits": out.logits.detach().numpy(),
           "emotion_logits": out.emotion_logits.detach().numpy(), "in_imgs": imgs.numpy()}
    for k, v in batch.items():
        rec["in_" + k] = v.numpy()
    for k, g in ref_g.items():
        rec["grad:" + k] = g.numpy()
    return rec


def dataset_case():
    """The reference's CustomDataset + PadCollate (src/custom_dataset.py:9-132) on synthetic pickles of
    the reference schema.  The reference keeps only the first dialogue of a file (its debugging
    ``[:1]`` slices, :21,27), so each dialogue is written to its own pair of pickles and the reference
    dataset is built once per dialogue; the concatenated samples are what a full run (slices removed,
    as its comment instructs) yields — the build's DialogueDataset processes every dialogue."""
    import pickle
    import tempfile
    from argparse import Namespace
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import custom_dataset as refds
    g = torch.Generator().manual_seed(77)
    eos, sp1, sp2, Fd = 50256, 50258, 50259, 8

    def toks(n):
        return torch.randint(0, 50257, (n,), generator=g).tolist()
    dialogues = []
    for i, shapes in enumerate([[(3, [5, 4, 6]), (4, [3, 3, 2, 7])], [(2, [9, 3])], [(2, [700, 400]), (1, [12])]]):
        txt, tgt, ctx, emo = [], [], [], []
        for j, (nt, lens) in enumerate(shapes):
            turns = [toks(n) for n in lens]
            txt.append(turns)
            # target lengths: shorter than, longer than and (the 1100-token utterance aside) like the input
            tl = {0: sum(lens) // 2, 1: sum(lens) + 5}.get((i + j) % 3, sum(lens) - 1)
            tgt.append([50257, sp1] + toks(max(tl, 1)) + [eos, eos])
            ctx.append(toks(6 + j))
            emo.append((3 * i + j) % 7)
        img = [torch.randn(Fd, generator=g).tolist()]
        aud = [torch.randn(Fd, generator=g).tolist()]
        dialogues.append(({"txt": [txt], "img": [img], "aud": [aud], "label": [tgt]},
                          {"context": [ctx], "label": [emo]}))
    samples = []
    tmp = tempfile.mkdtemp(prefix="ergm_ds_")
    for data, cl in dialogues:
        with open(os.path.join(tmp, "multi_train_data.pkl"), "wb") as f:
            pickle.dump(data, f)
        with open(os.path.join(tmp, "context_label_train_data.pkl"), "wb") as f:
            pickle.dump(cl, f)
        args = Namespace(train_prefix="train", valid_prefix="valid", data_dir=tmp, sp1_id=sp1, sp2_id=sp2, eos_id=eos)
        ds = refds.CustomDataset("train", args)
        samples += [ds[k] for k in range(len(ds))]
    collate = refds.PadCollate(eos, Namespace())
    batches = [collate.pad_collate(samples), collate.pad_collate(samples[1:3])]
    n = len(samples)
    Smax = max(len(x[0]) for x in samples)
    rec = {"n": np.array(n), "eos": np.array(eos), "sp1": np.array(sp1), "sp2": np.array(sp2),
           "lengths": np.array([len(x[0]) for x in samples]),
           "emotion": np.array([x[6] for x in samples]),
           "img0": np.array([x[3][0] for x in samples], dtype=np.float32),
           "aud0": np.array([x[4][0] for x in samples], dtype=np.float32),
           "n_img_rows": np.array([len(x[3]) for x in samples])}
    for key, col in (("input_ids", 0), ("token_type_ids", 1), ("labels", 2)):
        a = np.full((n, Smax), -7, dtype=np.int64)  # -7: beyond the sample
        for r, x in enumerate(samples):
            a[r, :len(x[col])] = x[col]
        rec["sample_" + key] = a
    ctx_len = max(len(x[5]) for x in samples)
    c = np.full((n, ctx_len), -7, dtype=np.int64)
    for r, x in enumerate(samples):
        c[r, :len(x[5])] = x[5]
    rec["sample_context"] = c
    for bi, b in enumerate(batches):
        for key, col in (("input_ids", 0), ("token_type_ids", 1), ("labels", 2)):
            rec[f"batch{bi}_" + key] = b[col].numpy()
    # the raw dialogues (the restatement's input)
    for i, (data, cl) in enumerate(dialogues):
        rec[f"dlg{i}_json"] = np.frombuffer(json.dumps({"data": data, "cl": cl}).encode(), dtype=np.uint8)
    print(f"  reference dataset: {n} samples from {len(dialogues)} dialogues (utterances >= 1024 tokens skipped)")
    return rec


def trainer_case(refmodel):
    """Three reference training steps of src/main.py's loop (:137-169: forward, zero_grad, backward,
    AdamW step, scheduler step, loss.item(), the no-grad LM cross-entropy over the logits, emotion
    argmax accuracy) with the poly-decay schedule (:93-95), then the epoch metrics (:171-176:
    mean loss, PPL = exp(mean LM loss), accuracy in %) and a validation pass (:206-251)."""
    import math
    import torch.nn as nn
    from transformers import GPT2Config, get_polynomial_decay_schedule_with_warmup
    cfg = O.OracleConfig(vocab_size=256, n_embd=64, n_layer=2, n_head=1, n_positions=64)
    seed = 66
    P = O.init_params(cfg, seed=seed)
    gcfg = GPT2Config(vocab_size=cfg.vocab_size, n_embd=cfg.n_embd, n_layer=cfg.n_layer, n_head=cfg.n_head,
                      n_positions=cfg.n_positions, attn_pdrop=0.0, resid_pdrop=0.0, embd_pdrop=0.0)
    net = refmodel.GPT2LMHeadModel(gcfg)
    sd = dict(P)
    sd["lm_head.weight"] = P["transformer.wte.weight"]
    net.load_state_dict(sd, strict=True)
    lr, steps = 1e-3, 3
    optim = torch.optim.AdamW(net.parameters(), lr=lr)
    sched = get_polynomial_decay_schedule_with_warmup(optim, num_warmup_steps=1, num_training_steps=steps, power=2)
    batches = [synthetic_batch(8, 16, n_turns=2, feat_dim=cfg.n_embd, seed=seed + 10 + k, vocab_hi=253, sp1=254,
                               sp2=255, eos=252) for k in range(steps + 1)]
    net.train()
    losses, lm_losses, correct, total = [], [], 0, 0
    for b in batches[:steps]:
        out = net(input_ids=b["input_ids"], token_type_ids=b["token_type_ids"], labels=b["labels"],
                  emotion_labels=b["emotion_labels"], caption_ids=b["caption_ids"], imgs=b["visual_feat"],
                  auds=b["audio_feat"])
        loss = out.loss
        optim.zero_grad()
        loss.backward()
        optim.step()
        sched.step()
        losses.append(loss.item())
        with torch.no_grad():
            sl = out.logits[..., :-1, :].contiguous()
            lab = b["labels"][..., 1:].contiguous()
            lm_losses.append(nn.CrossEntropyLoss()(sl.view(-1, sl.size(-1)), lab.view(-1)).item())
            correct += (torch.argmax(out.emotion_logits, dim=-1) == b["emotion_labels"]).sum().item()
            total += b["emotion_labels"].size(0)
    train = [float(np.mean(losses)), math.exp(float(np.mean(lm_losses))), correct / total * 100]
    net.eval()
    with torch.no_grad():
        b = batches[steps]
        out = net(input_ids=b["input_ids"], token_type_ids=b["token_type_ids"], labels=b["labels"],
                  emotion_labels=b["emotion_labels"], caption_ids=b["caption_ids"], imgs=b["visual_feat"],
                  auds=b["audio_feat"])
        sl = out.logits[..., :-1, :].contiguous()
        lab = b["labels"][..., 1:].contiguous()
        vlm = nn.CrossEntropyLoss()(sl.view(-1, sl.size(-1)), lab.view(-1)).item()
        vacc = (torch.argmax(out.emotion_logits, dim=-1) == b["emotion_labels"]).sum().item() / 8 * 100
        margins = out.emotion_logits.topk(2, dim=-1).values
        valid = [out.loss.item(), math.exp(vlm), vacc]
    print(f"  reference loop: train loss/ppl/acc {train}, valid {valid}")
    rec = {"config": np.array([cfg.vocab_size, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_positions]),
           "seed": np.array(seed), "lr": np.array(lr), "steps": np.array(steps),
           "step_losses": np.array(losses), "step_lm_losses": np.array(lm_losses),
           "train_metrics": np.array(train), "valid_metrics": np.array(valid),
           "valid_emotion_margin": (margins[:, 0] - margins[:, 1]).numpy()}
    for k, b in enumerate(batches):
        for n, v in b.items():
            rec[f"b{k}_{n}"] = v.numpy()
    return rec


def optim_case(refmodel):
    """The reference's optimizer state (src/main.py:68: ``torch.optim.AdamW(self.model.parameters())``,
    saved / resumed as ``optim_state_dict`` at :107,188): parameter order of ``model.parameters()`` (the
    tied lm_head dropped), the per-parameter ``exp_avg`` / ``exp_avg_sq`` / ``step`` after two reference
    training steps, the step-3 gradient, and the parameters and state after the third ``optim.step()``."""
    from transformers import GPT2Config
    cfg = O.OracleConfig(vocab_size=128, n_embd=64, n_layer=1, n_head=1, n_positions=32)
    seed = 77
    P = O.init_params(cfg, seed=seed)
    gcfg = GPT2Config(vocab_size=cfg.vocab_size, n_embd=cfg.n_embd, n_layer=cfg.n_layer, n_head=cfg.n_head,
                      n_positions=cfg.n_positions, attn_pdrop=0.0, resid_pdrop=0.0, embd_pdrop=0.0)
    net = refmodel.GPT2LMHeadModel(gcfg)
    sd = dict(P)
    sd["lm_head.weight"] = P["transformer.wte.weight"]
    net.load_state_dict(sd, strict=True)
    lr = 1e-3
    optim = torch.optim.AdamW(net.parameters(), lr=lr)
    names = {id(p): n for n, p in net.named_parameters()}
    order = [names[id(p)] for p in optim.param_groups[0]["params"]]
    batches = [synthetic_batch(4, 16, n_turns=2, feat_dim=cfg.n_embd, seed=seed + k, vocab_hi=125, sp1=126, sp2=127,
                               eos=124) for k in range(3)]
    net.train()
    rec = {"config": np.array([cfg.vocab_size, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_positions]),
           "seed": np.array(seed), "lr": np.array(lr),
           "param_order_json": np.frombuffer(json.dumps(order).encode(), dtype=np.uint8)}
    for k, b in enumerate(batches):
        out = net(input_ids=b["input_ids"], token_type_ids=b["token_type_ids"], labels=b["labels"],
                  emotion_labels=b["emotion_labels"], caption_ids=b["caption_ids"], imgs=b["visual_feat"],
                  auds=b["audio_feat"])
        optim.zero_grad()
        out.loss.backward()
        if k == 2:  # before the third step: the resumable state, the parameters and the gradient
            st = optim.state_dict()
            for i, n in enumerate(order):
                s = st["state"][i]
                rec[f"st2:{n}:exp_avg"] = s["exp_avg"].numpy().copy()
                rec[f"st2:{n}:exp_avg_sq"] = s["exp_avg_sq"].numpy().copy()
                rec[f"st2:{n}:step"] = np.array(float(s["step"]))
            for n, p in net.named_parameters():
                rec[f"p2:{n}"] = p.detach().numpy().copy()
                rec[f"g3:{n}"] = p.grad.detach().numpy().copy()
        optim.step()
    st = optim.state_dict()
    for i, n in enumerate(order):
        rec[f"st3:{n}:exp_avg"] = st["state"][i]["exp_avg"].numpy().copy()
        rec[f"st3:{n}:exp_avg_sq"] = st["state"][i]["exp_avg_sq"].numpy().copy()
    for n, p in net.named_parameters():
        rec[f"p3:{n}"] = p.detach().numpy().copy()
    g = st["param_groups"][0]
    rec["group_json"] = np.frombuffer(json.dumps({k: v for k, v in g.items() if k != "params"}).encode(),
                                      dtype=np.uint8)
    print(f"  reference AdamW over {len(order)} parameters, state after 3 steps recorded")
    return rec


XPEAK_E128 = (50.0, 50.0, 10.0)   # cross-attention scores std 2.5, mean max softmax probability 0.45 (vs 1/32 flat)
# GPT-2-small: scores std 1.4, mean max probability 0.12 (vs 1/128 flat).  Stronger gains amplify bf16 rounding
# through the 12 blocks beyond the bf16 gates for the reference itself: at (20, 20, 10) the reference under CPU bf16
# autocast deviates from its fp32 gradients by up to 6.9 % (rel-L2), at (15, 15, 5) by 1.8 %.
XPEAK_C2 = (15.0, 15.0, 5.0)


def xpeak_case(refmodel, name):
    """Peaked cross-attention: the reference's gradients with the caption-side projections
    scaled so the cross-attention softmax is far from uniform — no gradient is tiny against the model's scale, so
    the GPU gate holds every tensor, query side included, to the relative bound.  Two heads, full gradients at
    E = 128; norms and heads at the GPT-2-small C2 slice (12 heads, 12 blocks)."""
    if name == "xpeak_e128":
        cfg = O.OracleConfig(vocab_size=256, n_embd=128, n_layer=2, n_head=2, n_positions=64)
        _, _, rec = build_case(refmodel, name, cfg, B=2, S=32, seed=66, xpeak=XPEAK_E128)
    else:
        cfg = O.OracleConfig()
        _, _, rec = build_case(refmodel, name, cfg, B=2, S=128, seed=77, full_grads=False, vocab_hi=50257,
                               xpeak=XPEAK_C2)
    return rec


def main():
    torch.manual_seed(0)
    refmodel = load_reference()
    out_dir = HERE
    if "--only" in sys.argv:  # regenerate selected new fixtures without rewriting the older ones
        only = sys.argv[sys.argv.index("--only") + 1].split(",")
        cases = {"imgs2d": ("imgs2d_e64.npz", lambda: imgs2d_case(refmodel)),
                 "dataset": ("dataset_ref.npz", dataset_case),
                 "trainer": ("trainer_ref.npz", lambda: trainer_case(refmodel)),
                 "optim": ("optim_ref.npz", lambda: optim_case(refmodel)),
                 "xpeak": ("xpeak_e128.npz", lambda: xpeak_case(refmodel, "xpeak_e128")),
                 "xpeak_c2": ("xpeak_c2slice.npz", lambda: xpeak_case(refmodel, "xpeak_c2slice"))}
        for c in only:
            fn, make = cases[c]
            save_npz(os.path.join(out_dir, fn), make())  # in parts where one archive would pass 1 MiB
        return
    # 1. tiny, single head (d=64), full grads + one AdamW step: the byte-level fixture
    cfg = O.OracleConfig(vocab_size=256, n_embd=64, n_layer=2, n_head=1, n_positions=64)
    P, batch, rec = build_case(refmodel, "tiny_e64", cfg, B=2, S=32, seed=11)
    np.savez_compressed(os.path.join(out_dir, "tiny_e64.npz"), **rec)
    # 2. two heads, vocab not a multiple of 64, 4 visual rows (row 0 used), B=3
    cfg = O.OracleConfig(vocab_size=500, n_embd=128, n_layer=2, n_head=2, n_positions=128)
    _, _, rec = build_case(refmodel, "small_e128_v500", cfg, B=3, S=64, seed=22, visual_rows=4,
                           full_grads=False)
    np.savez_compressed(os.path.join(out_dir, "small_e128_v500.npz"), **rec)
    # 3. C1 shape: GPT-2-small text-only, B=2, S=128 (BASELINE configs[0]); stats only
    cfg = O.OracleConfig()
    _, _, rec = build_case(refmodel, "c1_gpt2small_textonly", cfg, B=2, S=128, seed=33,
                           with_features=False, full_grads=False, vocab_hi=50257)
    np.savez_compressed(os.path.join(out_dir, "c1_gpt2small_textonly.npz"), **rec)
    # 4. GPT-2-small + fusion, MELD shape, B=2 S=128 (a C2-shaped slice); stats only
    _, _, rec = build_case(refmodel, "c2slice_gpt2small_fusion", cfg, B=2, S=128, seed=44,
                           full_grads=False, vocab_hi=50257)
    np.savez_compressed(os.path.join(out_dir, "c2slice_gpt2small_fusion.npz"), **rec)
    np.savez_compressed(os.path.join(out_dir, "adamw_sched.npz"), **adamw_case())
    # 5. 2-D imgs (scalar imgs[i][0]), 6. the reference data pipeline, 7. the reference train loop's metrics
    np.savez_compressed(os.path.join(out_dir, "imgs2d_e64.npz"), **imgs2d_case(refmodel))
    np.savez_compressed(os.path.join(out_dir, "dataset_ref.npz"), **dataset_case())
    np.savez_compressed(os.path.join(out_dir, "trainer_ref.npz"), **trainer_case(refmodel))
    # 8. the reference optimizer's per-parameter state (checkpoint interchange)
    save_npz(os.path.join(out_dir, "optim_ref.npz"), optim_case(refmodel))
    print("golden fixtures written to", out_dir)


if __name__ == "__main__":
    main()
