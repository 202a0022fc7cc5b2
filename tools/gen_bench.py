"""Generation throughput and decode-attention bandwidth (recorded in DESIGN.md, not gated by any test).

Workload: GPT-2-small (random weights, so the nucleus is most of the vocabulary), prompt 64, captions 64, 64 new
tokens, top_p 0.95, an eos id no token has (every sequence runs to the bound).  tokens/s = B·64 over the time of the
whole call (prefill + sampling + decode), HIP events around it, 1 warm-up and the median of 5 repeats, for
  kv       KVCacheGenerator.nucleus_sampling, one sequence (the baseline)
  b1/8/32  BatchedGenerator.generate at B = 1, 8, 32 (engine "python": every launch enqueued from Python)
  n1/8/32  the same through the native decode executor on the same kernels (engine "native")
  f1/8/32  the executor on ergm_linear_rows (engine "fused"); with ERGM_DECODE_HEAD=lr or ln in the environment the
           LM head runs on that kernel too, behind ergm_layernorm_fwd (lr) or with the LayerNorm in its prologue (ln)
and ``attn``: ergm_attn_decode (append = 0, H = 12) at cache lengths 128 and 1,024 for B = 1 and 32, bytes/s = the
K/V bytes of the attended rows over the mean time of 200 back-to-back launches (median of 5 such windows), the
caches rotated through enough buffers to exceed the 256 MiB Infinity Cache where memory allows; set against the
6.3 TB/s an HBM copy reaches.  A window of back-to-back launches includes the launch gaps and the host's enqueue rate
(about 12-15 us per call from Python): for the kernel's own time run one shape under the profiler, in a run of its own,
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/gen_bench.py --case attn --shape 32,1024
and divide the same byte count by the mean duration of attn_decode_kernel (plus attn_decode_merge_kernel when the
automatic split is above 1).

Continuous batching: 256 requests, prompt 64, captions 64, each with its own max_new_tokens from one
seeded list, min(64, 1 + a geometric variable of mean 16): short on average with a long tail.  tokens/s = the requested
tokens (the sum of the list) over the whole call, and ``steps_per_token`` = decode steps executed per requested token.
  bs32/ns32/fs32  what a user does without it: BatchedGenerator.generate in arrival-order batches of 32 with the batch's
                  largest max_new_tokens, the lists truncated on the host (the baseline), per engine
  bc32/nc32/fc32  ContinuousGenerator(max_batch=32) on the same requests
  admit           one admission of n_seq = 1, 4, 8, 32 such prompts: milliseconds on engines "python" and "native" and
                  the native launch count; and the ragged attention launch against the n_seq ergm_attn_fwd launches it
                  replaces (causal, 64 rows each, H = 12), microseconds per call in back-to-back windows of 100
Conversations, ``turns``: 32 sessions of 4 turns, a 64-token first prompt, 16-token later turns and 16
new tokens per turn, on ContinuousGenerator(max_batch=32, max_len=192), engines "native" and "fused":
  continue   submit(keep=True), then extend_request per turn: each turn prefills its 16 new rows over the parked cache
  resubmit   what a user does without it: every turn is a new request carrying the whole history (the baseline)
tokens/s = the 2,048 requested tokens over the four turns of all sessions, the two ways alternating in one process,
median of 5 after a warm-up each; ``prefill_rows`` = the packed rows each turn's prefill ran over.
Sampling controls: the same 256 requests on ContinuousGenerator(controls=True),
  bd32/nd32/fd32  every request with the default SamplingParams (the new sampler, nothing asked of it)
  bx32/nx32/fx32  every request with top_k=50, temperature=0.8, repetition_penalty=1.2
and ``sample``: the sampler launch alone at B = 32, V = 50,257 on the logits an admission of 32 such prompts leaves,
microseconds per launch in back-to-back windows of 200, the variants alternating inside every repeat: ergm_topp_sample_rows
(old), ergm_sample_rows with no controls (defaults), top_k=50 only, repetition_penalty=1.2 only (the prompt's ids seen),
and everything (top_k=50, temperature=0.8, repetition_penalty=1.2).
Logit rules: the same 256 requests with controls=True and, on every request,
  br32/nr32/fr32  no_repeat_ngram_size=3          bw32/nw32/fw32  8 one-token bad words
against bd32/nd32/fd32 (controls only, the launches of before) in one ``--cases`` list, alternating.  The rules need an
eos inside the vocabulary, so these cases run with BEAM_EOS and count the tokens they produced.  ``--beams W --rules``
adds the ruled beam_search calls (n = 3; 8 one-token bad words) to the alternation of ``--beams W``.
Beam search, ``--beams W`` (W = 4 and W = 1 are recorded): G·W = 32 rows, 64 + 64 tokens, per engine the
milliseconds of one beam_search call beside one generate() call at B = 32 (alternating in one process; generate() and
everything under it are the parent commit's code, which the feature does not touch), the cache bytes the gather moved
per round, and the launches of a round alone in back-to-back windows of 200, alternating: select, the sampler launch
(ergm_topp_sample_rows), the gather of round 0 (W - 1 of W rows move) and a gather in which every beam keeps its row.
The whole runs in fresh child processes with ERGM_BEAM_SELECT=two and =one, alternating twice.
Beam search on the slots, ``--beams W --requests [--engines python,native,fused]``: the 256 requests by
beam search, per engine, as static arrival-order batches of 32 // W prompts (BatchedGenerator.beam_search, each batch to
its largest bound) and through one beam-mode ContinuousGenerator of 32 slots, alternating in one process, median of 5
after a warm-up: requested tokens/s, rounds and rounds per requested token of both, and the seed launch alone.
--case store: the session store.  First ergm_slots_save / ergm_slots_load against the "python"
engine's torch slicing for 1 / 8 / 32 sessions of 128 and 1,023 cache rows (HIP events, alternating, µs and GB/s of
bytes read + written); then 128 four-turn sessions on 32 slots with the turn shape of --case turns, the store against
re-submitting the history every turn, on "native" and "fused".
Without --case the tool runs every case in turn, each in a fresh child process under its own timeout, one at a
time, and stops at the first that fails.  --cases a,b,c runs those cases in that
order (e.g. b32,n32,f32,b32,n32,f32 to alternate engines on one box).  For the kernel-time split of one engine:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/gen_bench.py --case f32
Usage (GPU box): python tools/gen_bench.py [--case kv|b1|b8|b32|n*|f*|attn|bs32|bc32|bd32|bx32|n?32|f?32|admit|turns|sample|store]
                 [--cases LIST]"""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ENGINES = {"b": "python", "n": "native", "f": "fused"}
CASES = {"kv": 240, **{e + b: 240 for e in ENGINES for b in ("1", "8", "32")}, "attn": 240,   # seconds a child may take
         **{e + m + "32": 300 for e in ENGINES for m in "scdxrw"}, "admit": 240, "turns": 420, "sample": 240,
         "store": 1100}
N_REQ, REQ_MEAN = 256, 16
PROMPT = CAPS = NEW = 64
TOP_P, NO_EOS, SP2 = 0.95, -1, 50259
REPEATS = 5
EVERYTHING = dict(top_k=50, temperature=0.8, repetition_penalty=1.2)   # the controls of the x cases
BAD_WORDS = [[1000 * i + 7] for i in range(1, 9)]                      # the w cases: 8 one-token bad words
RULES = {"r": dict(no_repeat_ngram_size=3), "w": dict(bad_words_ids=BAD_WORDS)}


def _event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _generation(case):
    import torch
    from ergm_amd.config import ERGMConfig, NO_DROPOUT
    from ergm_amd.generate import BatchedGenerator, KVCacheGenerator
    from ergm_amd.model import GPT2LMHeadModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = GPT2LMHeadModel(ERGMConfig(**NO_DROPOUT), device=dev)
    B = 1 if case == "kv" else int(case[1:])
    g = torch.Generator().manual_seed(1)
    prompts = [(torch.randint(0, 50000, (1, PROMPT), generator=g).to(dev), torch.full((1, PROMPT), SP2, device=dev),
                torch.randint(0, 50000, (1, CAPS), generator=g).to(dev), None, None) for _ in range(B)]
    if case == "kv":
        def run():
            gen = KVCacheGenerator(model, max_len=PROMPT + NEW)
            out = gen.nucleus_sampling(*prompts[0][:3], top_p=TOP_P, eos_id=NO_EOS, sp2_id=SP2,
                                       generator=torch.Generator(device=dev).manual_seed(7))
            assert len(out) == NEW
    else:
        gen = BatchedGenerator(model, max_batch=B, max_len=PROMPT + NEW, engine=ENGINES[case[0]])

        def run():
            out = gen.generate(prompts, top_p=TOP_P, eos_id=NO_EOS, sp2_id=SP2, seed=7, max_new_tokens=NEW)
            assert all(len(r) == NEW for r in out)
    run()  # warm-up: code objects, GEMM plans, allocator
    ms = [_event_ms(run) for _ in range(REPEATS)]
    med = statistics.median(ms)
    print(json.dumps({"case": case, "engine": "single" if case == "kv" else ENGINES[case[0]], "B": B, "new_tokens": NEW, "ms_median": round(med, 2),
                      "ms_all": [round(x, 2) for x in ms], "tokens_per_s": round(B * NEW / med * 1e3, 1)}), flush=True)


def request_lengths(n):
    """The seeded max_new_tokens of the n requests: min(NEW, 2 + a geometric variable of mean 15).  Host only."""
    import torch
    geo = torch.distributions.Geometric(probs=torch.tensor(1.0 / REQ_MEAN))   # failures before a success: mean 15
    torch.manual_seed(2)
    return [min(NEW, 2 + int(geo.sample())) for _ in range(n)]                # 1 + a geometric variable of mean 16


def _setup_requests(n):
    import torch
    from ergm_amd.config import ERGMConfig, NO_DROPOUT
    from ergm_amd.model import GPT2LMHeadModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = GPT2LMHeadModel(ERGMConfig(**NO_DROPOUT), device=dev)
    g = torch.Generator().manual_seed(1)
    prompts = [(torch.randint(0, 50000, (1, PROMPT), generator=g).to(dev), torch.full((1, PROMPT), SP2, device=dev),
                torch.randint(0, 50000, (1, CAPS), generator=g).to(dev), None, None) for _ in range(n)]
    return dev, model, prompts, request_lengths(n)


def _requests(case):
    from ergm_amd.generate import BatchedGenerator, ContinuousGenerator, SamplingParams
    dev, model, prompts, new = _setup_requests(N_REQ)
    engine, B = ENGINES[case[0]], int(case[2:])
    steps, admits = [0], [N_REQ // B]
    if case[1] == "s":
        gen = BatchedGenerator(model, max_batch=B, max_len=PROMPT + NEW, engine=engine)

        def run():
            steps[0] = 0
            for i in range(0, N_REQ, B):
                k = max(new[i:i + B])
                out = gen.generate(prompts[i:i + B], top_p=TOP_P, eos_id=NO_EOS, sp2_id=SP2, seed=7, max_new_tokens=k)
                out = [r[:m] for r, m in zip(out, new[i:i + B])]
                assert [len(r) for r in out] == new[i:i + B]
                steps[0] += k - 1
    else:
        gen = ContinuousGenerator(model, max_batch=B, max_len=PROMPT + NEW, cap_max=CAPS, engine=engine,
                                  controls=case[1] in "dxrw")
        sampling = {"c": None, "d": SamplingParams(), "x": SamplingParams(**EVERYTHING),
                    **{k: SamplingParams(**v) for k, v in RULES.items()}}[case[1]]
        ruled = case[1] in RULES
        produced = [sum(new)]

        def run():
            s0, a0 = gen.sched.steps, gen.admit_calls
            out = gen.generate(prompts, top_p=TOP_P, eos_id=BEAM_EOS if ruled else NO_EOS, sp2_id=SP2, seed=7,
                               max_new_tokens=new, sampling=sampling)
            if ruled:   # an eos inside the vocabulary can be drawn: count what came out
                assert all(1 <= len(r) <= m for r, m in zip(out, new))
                produced[0] = sum(len(r) for r in out)
            else:
                assert [len(r) for r in out] == new
            steps[0], admits[0] = gen.sched.steps - s0, gen.admit_calls - a0
    run()
    ms = [_event_ms(run) for _ in range(REPEATS)]
    med = statistics.median(ms)
    print(json.dumps({"case": case, "engine": engine, "B": B, "requests": N_REQ, "requested_tokens": sum(new),
                      "max_new_mean": round(sum(new) / N_REQ, 2), "max_new_max": max(new), "decode_steps": steps[0],
                      "steps_per_token": round(steps[0] / sum(new), 4),
                      "admit_calls": admits[0], "ms_median": round(med, 2),
                      "ms_all": [round(x, 2) for x in ms], "produced_tokens": produced[0],
                      "tokens_per_s": round(produced[0] / med * 1e3, 1)}), flush=True)


def _admission():
    import torch
    from ergm_amd import ops
    from ergm_amd.generate import ContinuousGenerator
    dev, model, prompts, _ = _setup_requests(32)
    H, E, N = 12, 768, 100
    for n in (1, 4, 8, 32):
        row = {"case": "admit", "n_seq": n, "rows": n * PROMPT}
        for engine in ("python", "native"):
            gen = ContinuousGenerator(model, max_batch=32, max_len=PROMPT + NEW, cap_max=CAPS, engine=engine)
            run = lambda: gen.admit(list(range(n)), prompts[:n])
            run()
            row[f"{engine}_ms"] = round(statistics.median(_event_ms(run) for _ in range(REPEATS)), 3)
            if engine == "native":
                row["native_launches"] = gen.admit_launches(n, n * PROMPT, n * CAPS)
        # one ragged launch against n ergm_attn_fwd launches over the same packed qkv rows
        qkv = torch.randn(n * PROMPT, 3 * E, device=dev).bfloat16()
        o = torch.empty(n * PROMPT, E, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(H * n * PROMPT, dtype=torch.float32, device=dev)
        st = torch.arange(0, n * PROMPT, PROMPT, dtype=torch.int32, device=dev)
        ln = torch.full((n,), PROMPT, dtype=torch.int32, device=dev)

        def ragged():
            for _ in range(N):
                ops.attn_fwd_ragged(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], st, ln, st, ln, H, PROMPT, PROMPT, True, o=o)

        def per_seq():
            for _ in range(N):
                for b in range(n):
                    r = slice(b * PROMPT, (b + 1) * PROMPT)
                    ops.attn_fwd(qkv[r, :E], qkv[r, E:2 * E], qkv[r, 2 * E:], 1, H, PROMPT, PROMPT, True, o=o[r],
                                 lse=lse[:H * PROMPT].view(1, H, PROMPT))
        for name, fn in (("ragged_us", ragged), ("per_sequence_us", per_seq)):
            fn()
            row[name] = round(statistics.median(_event_ms(fn) for _ in range(REPEATS)) / N * 1e3, 2)
        print(json.dumps(row), flush=True)


def _sampler():
    import torch
    from ergm_amd import ops
    from ergm_amd.generate import ContinuousGenerator
    dev, model, prompts, _ = _setup_requests(32)
    B, N = 32, 200
    gen = ContinuousGenerator(model, max_batch=B, max_len=PROMPT + NEW, cap_max=CAPS, engine="native")
    gen.admit(list(range(B)), prompts)
    logits, V = gen._logits, 50257   # GPT-2's own vocabulary: the model's added special tokens stay out of the draw
    rid = torch.arange(B, dtype=torch.int32, device=dev)
    steps = torch.zeros(B, dtype=torch.int32, device=dev)
    tokens = torch.empty(B, dtype=torch.int64, device=dev)
    f = lambda v: torch.full((B,), v, dtype=torch.float32, device=dev)
    top_k, temp, pen = torch.full((B,), EVERYTHING["top_k"], dtype=torch.int32, device=dev), f(EVERYTHING["temperature"]), \
        f(EVERYTHING["repetition_penalty"])

    def bitmap():   # the prompts' ids, as an admission marks them
        seen = torch.zeros(B, (V + 31) // 32, dtype=torch.int32, device=dev)
        ids = torch.cat([p[0].reshape(-1) for p in prompts])
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        ops.sample_mark(ids, i32(list(range(B))), i32([b * PROMPT for b in range(B)]), i32([PROMPT] * B), V, seen=seen)
        return seen
    ctls = {"defaults": None, "top_k": ops.sample_ctl(top_k=top_k), "penalty": ops.sample_ctl(rep_penalty=pen, seen=bitmap()),
            "everything": ops.sample_ctl(top_k=top_k, temperature=temp, rep_penalty=pen, seen=bitmap())}

    def window(name):
        def run():
            for _ in range(N):
                if name == "old":
                    ops.topp_sample_rows(logits, V, TOP_P, 7, rid, steps, NO_EOS, tokens=tokens)
                else:
                    ops.sample_rows(logits, V, TOP_P, 7, rid, steps, NO_EOS, ctl=ctls[name], tokens=tokens)
        return run
    names = ["old", *ctls]
    us = {n: [] for n in names}
    for rep in range(REPEATS + 1):   # alternating; the first of each is the warm-up
        for n in names:
            t = _event_ms(window(n)) / N * 1e3
            if rep:
                us[n].append(t)
    for n in names:
        print(json.dumps({"case": "sample", "variant": n, "B": B, "V": V, "us_per_launch": round(statistics.median(us[n]), 2),
                          "us_all": [round(x, 2) for x in us[n]]}), flush=True)


SESSIONS, TURNS, TURN_ROWS, TURN_NEW = 32, 4, 16, 16


def _turns():
    import torch
    from ergm_amd.generate import ContinuousGenerator
    dev, model, prompts, _ = _setup_requests(SESSIONS)
    g = torch.Generator().manual_seed(3)
    later = [[(torch.randint(0, 50000, (TURN_ROWS,), generator=g).to(dev), torch.full((TURN_ROWS,), SP2 - 1, device=dev))
              for _ in range(SESSIONS)] for _ in range(TURNS - 1)]
    max_len = PROMPT + TURN_NEW + (TURNS - 1) * (TURN_ROWS + TURN_NEW)
    max_len = (max_len + 63) // 64 * 64
    for engine in ("native", "fused"):
        gen = ContinuousGenerator(model, max_batch=SESSIONS, max_len=max_len, cap_max=CAPS, engine=engine)
        rows = {"continue": [], "resubmit": []}
        sample = dict(top_p=TOP_P, eos_id=NO_EOS, sp2_id=SP2, seed=7)

        def run_continue():
            rows["continue"] = [SESSIONS * PROMPT] + [SESSIONS * TURN_ROWS] * (TURNS - 1)
            ids = [gen.submit(p, TURN_NEW, keep=True) for p in prompts]
            out = gen.run(**sample)
            for t in range(TURNS - 1):
                for i, (x, tt) in zip(ids, later[t]):
                    gen.extend_request(i, x, tt, TURN_NEW)
                out = gen.run(**sample)
                assert all(len(out[i]) == TURN_NEW for i in ids)
            for i in ids:
                gen.release(i)

        def run_resubmit():
            hist = [(p[0], p[1]) for p in prompts]
            rows["resubmit"] = []
            for t in range(TURNS):
                if t:
                    hist = [(torch.cat([h[0], torch.tensor([new[i]], device=dev), later[t - 1][b][0].view(1, -1)], 1),
                             torch.cat([h[1], torch.full((1, TURN_NEW), SP2, device=dev), later[t - 1][b][1].view(1, -1)], 1))
                            for b, (h, i) in enumerate(zip(hist, ids))]
                rows["resubmit"].append(sum(int(h[0].numel()) for h in hist))
                ids = [gen.submit((h[0], h[1], p[2], None, None), TURN_NEW) for h, p in zip(hist, prompts)]
                new = gen.run(**sample)
                assert all(len(new[i]) == TURN_NEW for i in ids)

        ms = {"continue": [], "resubmit": []}
        for rep in range(REPEATS + 1):   # alternating; the first of each is the warm-up
            for name, fn in (("continue", run_continue), ("resubmit", run_resubmit)):
                t = _event_ms(fn)
                if rep:
                    ms[name].append(t)
        tokens = SESSIONS * TURNS * TURN_NEW
        row = {"case": "turns", "engine": engine, "sessions": SESSIONS, "turns": TURNS, "requested_tokens": tokens,
               "extend_launches": gen.extend_launches(SESSIONS, SESSIONS * TURN_ROWS)}
        for name in ms:
            med = statistics.median(ms[name])
            row[name] = {"ms_median": round(med, 2), "ms_all": [round(x, 2) for x in ms[name]],
                         "tokens_per_s": round(tokens / med * 1e3, 1), "prefill_rows": rows[name]}
        row["speedup"] = round(statistics.median(ms["resubmit"]) / statistics.median(ms["continue"]), 3)
        print(json.dumps(row), flush=True)


STORE_SESSIONS, STORE_SLOTS = 128, 32


def _store_kernels(dev, model):
    """ergm_slots_save / ergm_slots_load against the "python" engine's torch slicing, HIP events, alternating: n sessions
    of `rows` cache rows and CAPS caption rows of GPT-2 small; bytes = what a save reads and writes."""
    import torch
    from ergm_amd.generate import ContinuousGenerator
    for rows in (128, 1023):
        gens = {e: ContinuousGenerator(model, max_batch=32, max_len=1024, cap_max=CAPS, engine=e, session_store=True)
                for e in ("python", "native")}
        for g in gens.values():
            for t in g.kv + g.xkv:
                t.normal_()
        for n in (1, 8, 32):
            slots, ids = list(range(n)), list(range(n))
            ms = {(e, op): [] for e in gens for op in ("save", "load")}
            for rep in range(REPEATS + 1):
                for e, g in gens.items():
                    t_save = _event_ms(lambda: g.save_sessions(slots, ids, rows=[rows] * n, cap_rows=[CAPS] * n))
                    t_load = _event_ms(lambda: g.load_sessions(slots, ids))
                    nbytes = g.stored_bytes
                    for i in ids:
                        g.drop_session(i)
                    if rep:
                        ms[(e, "save")].append(t_save)
                        ms[(e, "load")].append(t_load)
            row = {"case": "store_kernels", "sessions": n, "rows": rows, "cap_rows": CAPS, "blob_bytes": nbytes}
            for (e, op), v in ms.items():
                med = statistics.median(v)
                row[f"{e}_{op}"] = {"us_median": round(med * 1e3, 1), "us_all": [round(x * 1e3, 1) for x in v],
                                    "GB_per_s": round(2 * nbytes / med / 1e6, 1)}
            print(json.dumps(row), flush=True)


def _store():
    """128 four-turn sessions on 32 slots with the turn shape of --case turns: the session store against re-submitting
    the whole history every turn, which is all a generator without a store offers for more sessions than slots."""
    import torch
    from ergm_amd.generate import ContinuousGenerator
    dev, model, prompts, _ = _setup_requests(STORE_SESSIONS)
    _store_kernels(dev, model)
    g = torch.Generator().manual_seed(3)
    later = [[(torch.randint(0, 50000, (TURN_ROWS,), generator=g).to(dev), torch.full((TURN_ROWS,), SP2 - 1, device=dev))
              for _ in range(STORE_SESSIONS)] for _ in range(TURNS - 1)]
    max_len = (PROMPT + TURN_NEW + (TURNS - 1) * (TURN_ROWS + TURN_NEW) + 63) // 64 * 64
    sample = dict(top_p=TOP_P, eos_id=NO_EOS, sp2_id=SP2, seed=7)
    for engine in ("native", "fused"):
        kw = dict(max_batch=STORE_SLOTS, max_len=max_len, cap_max=CAPS, engine=engine)
        stored, plain = ContinuousGenerator(model, session_store=True, **kw), ContinuousGenerator(model, **kw)
        moved = [0]

        def run_store():
            c0 = (stored.save_calls, stored.load_calls)
            moved[0] = 0
            ids = [stored.submit(p, TURN_NEW, keep=True) for p in prompts]
            stored.run(**sample)
            for t in range(TURNS - 1):
                for i, (x, tt) in zip(ids, later[t]):
                    stored.extend_request(i, x, tt, TURN_NEW)
                out = stored.run(**sample)
                assert all(len(out[i]) == TURN_NEW for i in ids)
            moved[0] = stored.stored_bytes   # what the store holds when the last turn has run
            for i in ids:
                stored.release(i)
            return stored.save_calls - c0[0], stored.load_calls - c0[1]

        def run_resubmit():
            hist = [(p[0], p[1]) for p in prompts]
            for t in range(TURNS):
                if t:
                    hist = [(torch.cat([h[0], torch.tensor([new[i]], device=dev), later[t - 1][b][0].view(1, -1)], 1),
                             torch.cat([h[1], torch.full((1, TURN_NEW), SP2, device=dev), later[t - 1][b][1].view(1, -1)], 1))
                            for b, (h, i) in enumerate(zip(hist, ids))]
                ids = [plain.submit((h[0], h[1], p[2], None, None), TURN_NEW) for h, p in zip(hist, prompts)]
                new = plain.run(**sample)
                assert all(len(new[i]) == TURN_NEW for i in ids)

        ms, calls = {"store": [], "resubmit": []}, (0, 0)
        for rep in range(REPEATS + 1):   # alternating; the first of each is the warm-up
            for name, fn in (("store", run_store), ("resubmit", run_resubmit)):
                res = []
                t = _event_ms(lambda: res.append(fn()))
                if name == "store":
                    calls = res[0]
                if rep:
                    ms[name].append(t)
        tokens = STORE_SESSIONS * TURNS * TURN_NEW
        row = {"case": "store", "engine": engine, "sessions": STORE_SESSIONS, "slots": STORE_SLOTS, "turns": TURNS,
               "requested_tokens": tokens, "save_calls": calls[0], "load_calls": calls[1], "stored_bytes_at_end": moved[0]}
        for name in ms:
            med = statistics.median(ms[name])
            row[name] = {"ms_median": round(med, 2), "ms_all": [round(x, 2) for x in ms[name]],
                         "tokens_per_s": round(tokens / med * 1e3, 1)}
        row["speedup"] = round(statistics.median(ms["resubmit"]) / statistics.median(ms["store"]), 3)
        print(json.dumps(row), flush=True)


BEAM_EOS = 50258   # a special token the random model's beams do not reach: every search runs to the bound


def _beams(W):
    """One child of --beams W: beam_search against generate() per engine, and the launches of a round alone."""
    import torch
    from ergm_amd import ops
    from ergm_amd.generate import BatchedGenerator
    R, N = 32, 200
    dev, model, prompts, _ = _setup_requests(R)
    G = R // W
    mode = os.environ.get("ERGM_BEAM_SELECT", "two")
    kv_row = 2 * model.config.n_embd * 2
    for engine in ENGINES.values():
        gen_b = BatchedGenerator(model, max_batch=R, max_len=PROMPT + NEW, engine=engine)
        gen_p = BatchedGenerator(model, max_batch=R, max_len=PROMPT + NEW, engine=engine)

        def beam():
            out = gen_b.beam_search(prompts[:G], W, BEAM_EOS, SP2, max_new_tokens=NEW)
            assert all(len(h[0][0]) == NEW for h in out)

        def plain():   # the parent commit's call: generate() and everything under it are unchanged by this feature
            out = gen_p.generate(prompts, top_p=TOP_P, eos_id=NO_EOS, sp2_id=SP2, seed=7, max_new_tokens=NEW)
            assert all(len(r) == NEW for r in out)
        ms = {"beam": [], "plain": []}
        fns = [("beam", beam), ("plain", plain)]
        if "--rules" in sys.argv:
            for key, kw in RULES.items():
                def ruled(kw=kw):
                    out = gen_b.beam_search(prompts[:G], W, BEAM_EOS, SP2, max_new_tokens=NEW, **kw)
                    assert all(1 <= len(h[0][0]) <= NEW for h in out)
                fns.append(("beam_" + key, ruled))
                ms["beam_" + key] = []
        for rep in range(REPEATS + 1):   # alternating; the first of each is the warm-up
            for name, fn in fns:
                t = _event_ms(fn)
                if rep:
                    ms[name].append(t)
        # the cache bytes the gather moved: a row that changed parents copies the rows its parent held
        gen_b.beam_prefill(prompts[:G], W, BEAM_EOS, SP2)
        _, parents = gen_b.beam_round(NEW)
        moved = [sum(1 for r, p in enumerate(par) if p != r) * (PROMPT + i) * kv_row * model.config.n_layer
                 for i, par in enumerate(parents)]
        print(json.dumps({"case": "beams", "select": mode, "engine": engine, "W": W, "G": G, "new_tokens": NEW,
                          "beam_ms_median": round(statistics.median(ms["beam"]), 2), "beam_ms_all": [round(x, 2) for x in ms["beam"]],
                          **{k + "_ms_median": round(statistics.median(v), 2) for k, v in ms.items() if k.startswith("beam_")},
                          **{k + "_ms_all": [round(x, 2) for x in v] for k, v in ms.items() if k.startswith("beam_")},
                          "generate_ms_median": round(statistics.median(ms["plain"]), 2),
                          "generate_ms_all": [round(x, 2) for x in ms["plain"]],
                          "gather_bytes_round0": moved[0], "gather_bytes_per_round_mean_later": round(sum(moved[1:]) / (NEW - 1)),
                          "rows_moved_per_round_mean_later": round(sum(sum(1 for r, p in enumerate(par) if p != r)
                                                                       for par in parents[1:]) / (NEW - 1), 2)}), flush=True)
    # the launches alone, on the state a search holds after its first round (every row live, 65 cache rows)
    gen = BatchedGenerator(model, max_batch=R, max_len=PROMPT + NEW, engine="native")
    gen.beam_prefill(prompts[:G], W, BEAM_EOS, SP2)
    gen.beam_round(1)
    logits, V = gen._logits, model.layout.vocab
    scores0, sc = gen.beam_scores.clone(), gen.beam_scores.clone()
    fin = torch.zeros(R, dtype=torch.uint8, device=dev)
    par, tok = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int64, device=dev)
    rid, steps = torch.arange(R, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
    fan = torch.arange(R, dtype=torch.int32, device=dev) // W * W            # round 0: W - 1 of W rows move
    keep = torch.arange(R, dtype=torch.int32, device=dev)                    # every beam keeps its row
    lens = gen.lens.clone()

    def select():
        sc.copy_(scores0), fin.zero_()
        for _ in range(N):
            ops.beam_select(logits, V, W, sc, fin, BEAM_EOS, parent=par, token=tok, ws=gen._beam_ws)

    def sampler():
        for _ in range(N):
            ops.topp_sample_rows(logits, V, TOP_P, 7, rid, steps, NO_EOS, tokens=tok)

    def gather(p):
        def run():
            for _ in range(N):
                ops.beam_gather(gen.kv, p, lens, W, max_len=gen.n_max)
        return run
    fns = {"select": select, "sampler": sampler, "gather_fan_out": gather(fan), "gather_none": gather(keep)}
    us = {n: [] for n in fns}
    for rep in range(REPEATS + 1):
        for n, fn in fns.items():
            t = _event_ms(fn) / N * 1e3
            if rep:
                us[n].append(t)
    fan_bytes = int((fan != keep).sum()) * int(lens[0]) * kv_row * model.config.n_layer
    for n in fns:
        print(json.dumps({"case": "beams", "select": mode, "launch": n, "W": W, "R": R, "V": V,
                          "us_per_call": round(statistics.median(us[n]), 2), "us_all": [round(x, 2) for x in us[n]],
                          **({"bytes": fan_bytes, "cache_rows": int(lens[0])} if n == "gather_fan_out" else {})}), flush=True)


def _beam_requests(W):
    """--beams W --requests: the 256-request list by beam search, per engine, served two ways that alternate in one
    process: static (BatchedGenerator.beam_search in arrival-order batches of 32 // W prompts, each with its largest
    bound: the static path of Trainer.test) and continuous (a beam-mode ContinuousGenerator of 32 slots).  Then the seed
    launch alone, for one group and for all of them."""
    import torch
    from ergm_amd import ops
    from ergm_amd.generate import BatchedGenerator, ContinuousGenerator
    R = 32
    G = R // W
    dev, model, prompts, new = _setup_requests(N_REQ)
    only = sys.argv[sys.argv.index("--engines") + 1].split(",") if "--engines" in sys.argv else list(ENGINES.values())
    for engine in only:
        gen_s = BatchedGenerator(model, max_batch=R, max_len=PROMPT + NEW, engine=engine)
        gen_c = ContinuousGenerator(model, max_batch=R, max_len=PROMPT + NEW, cap_max=CAPS, engine=engine, num_beams=W)
        rounds = {"static": 0, "continuous": 0}
        calls = {"admit": 0, "seed": 0}

        def static():
            rounds["static"] = 0
            for i in range(0, N_REQ, G):
                k = max(new[i:i + G])
                out = gen_s.beam_search(prompts[i:i + G], W, BEAM_EOS, SP2, max_new_tokens=k)
                assert all(len(h[0][0]) == k for h in out)
                rounds["static"] += k

        def continuous():
            s0, a0, d0 = gen_c.sched.steps, gen_c.admit_calls, gen_c.seed_calls
            out = gen_c.beam_search(prompts, BEAM_EOS, SP2, max_new_tokens=new)
            assert [len(h[0][0]) for h in out] == new
            rounds["continuous"] = gen_c.sched.steps - s0
            calls["admit"], calls["seed"] = gen_c.admit_calls - a0, gen_c.seed_calls - d0
        ms = {"static": [], "continuous": []}
        for rep in range(REPEATS + 1):   # alternating; the first of each is the warm-up
            for name, fn in (("static", static), ("continuous", continuous)):
                t = _event_ms(fn)
                if rep:
                    ms[name].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"case": "beam_requests", "engine": engine, "W": W, "groups": G, "requests": N_REQ,
                          "requested_tokens": sum(new),
                          **{f"{k}_ms_median": round(med[k], 2) for k in ms}, **{f"{k}_ms_all": [round(x, 2) for x in ms[k]] for k in ms},
                          **{f"{k}_tokens_per_s": round(sum(new) / med[k] * 1e3, 1) for k in ms},
                          **{f"{k}_rounds": rounds[k] for k in ms},
                          **{f"{k}_rounds_per_token": round(rounds[k] / sum(new), 4) for k in ms},
                          "admit_calls": calls["admit"], "seed_calls": calls["seed"],
                          "speedup": round(med["static"] / med["continuous"], 3)}), flush=True)
    # the seed launch alone, behind an admission of every group
    gen = ContinuousGenerator(model, max_batch=R, max_len=PROMPT + NEW, cap_max=CAPS, engine="native", num_beams=W)
    gen.admit_beams(list(range(G)), prompts[:G])
    N = 200
    for groups in ([0], list(range(G))):
        gdev = torch.tensor(groups, dtype=torch.int32, device=dev)

        def seed():
            for _ in range(N):
                ops.beam_seed(gen.xkv, groups, W, CAPS, gen.lens, gen.cap_lens, gen.stop_lens, gen.finished, gen.beam_scores,
                              groups_dev=gdev)
        seed()
        us = [_event_ms(seed) / N * 1e3 for _ in range(REPEATS)]
        kv_row = 2 * model.config.n_embd * 2
        print(json.dumps({"case": "beam_requests", "launch": "seed", "W": W, "groups": len(groups),
                          "bytes": len(groups) * (W - 1) * CAPS * kv_row * model.config.n_layer,
                          "us_per_call": round(statistics.median(us), 2), "us_all": [round(x, 2) for x in us]}), flush=True)


def _attention():
    import torch
    from ergm_amd import ops
    dev = torch.device("cuda:0")
    H, E, N = 12, 768, 200
    only = sys.argv[sys.argv.index("--shape") + 1].split(",") if "--shape" in sys.argv else None
    for B in (1, 32):
        for n in (128, 1024):
            if only and [str(B), str(n)] != only:
                continue
            nbytes = B * n * 2 * E * 2
            nbuf = max(1, min(8, -(-(512 << 20) // nbytes)))
            caches = [torch.randn(B, n, 2 * E, device=dev).bfloat16() for _ in range(nbuf)]
            q = torch.randn(B, E, device=dev).bfloat16()
            lens = torch.full((B,), n, dtype=torch.int32, device=dev)
            ws = ops.attn_decode_workspace(B, H, n, dev)
            out = torch.empty(B, E, dtype=torch.bfloat16, device=dev)

            def window():
                for i in range(N):
                    c = caches[i % nbuf]
                    ops.attn_decode(q, c[:, :, :E], c[:, :, E:], lens, False, out=out, ws=ws)
            window()
            us = statistics.median(_event_ms(window) for _ in range(REPEATS)) / N * 1e3
            print(json.dumps({"case": "attn", "B": B, "cache_len": n, "kv_bytes": nbytes, "buffers": nbuf,
                              "us_per_launch": round(us, 2), "TB_per_s": round(nbytes / us / 1e6, 3),
                              "share_of_6.3TBps": round(nbytes / us / 1e6 / 6.3, 3)}), flush=True)


def main():
    if "--beams" in sys.argv:
        W = int(sys.argv[sys.argv.index("--beams") + 1])
        if not 1 <= W <= 8 or 32 % W:
            raise SystemExit("--beams takes 1, 2, 4 or 8")
        if "--requests" in sys.argv:   # one process: the two ways alternate inside it
            return _beam_requests(W)
        if "--child" in sys.argv:
            return _beams(W)
        for mode in ("two", "one", "two", "one"):   # the two forms of select, alternating, a fresh process each
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--beams", str(W), "--child",
                                *(["--rules"] if "--rules" in sys.argv else [])], timeout=420,
                               env={**os.environ, "ERGM_BEAM_SELECT": mode})
            if r.returncode != 0:
                raise SystemExit(f"--beams {W} (select {mode}) failed with status {r.returncode}: stopping")
        return
    if "--case" in sys.argv:
        case = sys.argv[sys.argv.index("--case") + 1]
        if case not in CASES:
            raise SystemExit(f"unknown case {case}")
        if case == "attn":
            _attention()
        elif case == "admit":
            _admission()
        elif case == "turns":
            _turns()
        elif case == "sample":
            _sampler()
        elif case == "store":
            _store()
        elif len(case) == 4 and case[1] in "scdxrw":
            _requests(case)
        else:
            _generation(case)
        return
    order = sys.argv[sys.argv.index("--cases") + 1].split(",") if "--cases" in sys.argv else list(CASES)
    for case in order:
        if case not in CASES:
            raise SystemExit(f"unknown case {case}")
        limit = CASES[case]
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"case {case} exceeded {limit} s: stopping")
        if r.returncode != 0:
            raise SystemExit(f"case {case} failed with status {r.returncode}: stopping")


if __name__ == "__main__":
    main()
