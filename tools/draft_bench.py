"""What draft verification is worth, host call to return -> profiles/draft_bench.json (a record, not a test; DESIGN.md 6.11 quotes it).

Full dimensions, synthetic weights, B = 1, one 20 s segment, 150 tokens.  The request's own greedy ids, cut to 0 / 50 / 100 / 149 tokens, are its draft - with one
wrong id appended where the draft is shorter than the transcript, so that the verify pass always ends on a rejection, as a real draft does.  With synthetic weights
the speed-up says what a draft that is right up to that point saves; how much of a real draft is right is the caller's affair.
  engine    Engine.transcribe_batch of the one request per draft length: wall time, the device's stage times (sonic_timings), the accepted count
  model     16 such requests through ASRModel.submit (the native continuous dispatcher), drafts of 0 and of 149 tokens: wall time until the last future resolves
Wall times: warm-up rounds, then the forms alternating round by round; median, 10th / 90th percentile and the count.  The added buffers are sonic_memory_info before
and after the handle's first drafted prefill.  Nothing is asserted.

    python tools/draft_bench.py [--rounds 7] [--warmup 2] [--tokens 150] [--tiny]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sonicscribe_amd import spec, synth  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs) * 1e3, 3), "p10_ms": round(xs[len(xs) // 10] * 1e3, 3), "p90_ms": round(xs[(len(xs) * 9) // 10] * 1e3, 3), "n": len(xs)}


def alternate(forms, warmup, rounds):
    t, last = {k: [] for k, _ in forms}, {}
    for r in range(warmup + rounds):
        k = r % len(forms)
        for name, fn in forms[k:] + forms[:k]:
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            if r >= warmup:
                t[name].append(dt)
                last[name] = out
    return {k: spread(v) for k, v in t.items()}, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=150)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draft_bench.json"))
    a = ap.parse_args()
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.engine import Engine
    d = spec.TINY if a.tiny else spec.FULL
    n_tok, n = a.tokens, int(a.seconds * 16000)
    cuts = sorted({0, n_tok // 3, 2 * n_tok // 3, n_tok - 1})
    pcm = synth.synth_pcm(100, n)
    prompt = [1, 17, 23, 5] + [d.audio_token_id] * spec.audio_token_count(spec.valid_frames(n)) + [7, 301, 302, 303, 9, 11]
    eng = Engine(d, 0, 0, max_batch=8, max_ctx=1024)
    eng.set_option("token_logprobs", 1)
    eng.set_option("draft_verify", 1)
    eng.load_synthetic(20260128)
    own = [int(t) for t in eng.transcribe_batch([pcm], [prompt], [n_tok])[0][0]]
    banned = set(d.eos_ids) | {d.audio_token_id}
    full = [t for t in own if t not in banned]                       # (a transcript that ended on EOS: the draft stops in front of it)

    def draft(k):
        if k == 0:
            return []                                                # the undrafted request: nothing is staged
        dr = full[:k]
        if k < min(len(full), n_tok - 1):
            wrong = next(t for t in range(5, d.vocab) if t not in banned and t != full[k])
            dr = dr + [wrong]
        return dr
    mem0 = eng.memory_info()[0]
    eng.transcribe_batch([pcm], [prompt], [n_tok], request_draft=[draft(cuts[1])])
    added = eng.memory_info()[0] - mem0

    def run(k):
        def f():
            ids, _ = eng.transcribe_batch([pcm], [prompt], [n_tok], request_draft=[draft(k)] if k else None)
            t = eng.timings()
            return {"accepted": int(eng.draft_accepted(1)[0]), "tokens": len(ids[0]), "equal_to_undrafted": int(np.sum(np.asarray(ids[0][:len(own)]) == np.asarray(own[:len(ids[0])]))),
                    "prefill_ms": round(t["prefill_ms"], 3), "decode_ms": round(t["decode_ms"], 3), "decode_steps": int(t["decode_steps"]), "total_ms": round(t["total_ms"], 3)}
        return f
    wall, last = alternate([(f"draft_{k}", run(k)) for k in cuts], a.warmup, a.rounds)
    res = {"dims": "tiny" if a.tiny else "full", "seconds": a.seconds, "tokens": n_tok, "transcript_tokens": len(own), "draft_lengths": {f"draft_{k}": len(draft(k)) for k in cuts},
           "added_buffer_bytes": int(added), "engine_wall": wall, "engine_device": last}
    eng.close()

    m = ASRModel.from_synthetic(d, 20260128, max_batch=32, max_ctx=1024, token_logprobs=True, draft_verify=True)
    wav = pcm.astype(np.float32) / 32768.0
    base = m.submit(wav, max_new_tokens=n_tok, detailed=True).result()
    mine = [int(t) for t in base.token_ids if int(t) not in banned][:n_tok - 1]

    def burst(dr):
        def f():
            futs = [m.submit(wav, max_new_tokens=n_tok, detailed=True, draft=dr) for _ in range(16)]
            out = [x.result() for x in futs]
            return {"draft_len": out[0].draft_len, "draft_matched": out[0].draft_matched, "tokens": int(out[0].token_ids.size)}
        return f
    wall, last = alternate([("no_draft", burst(None)), ("draft_all_but_one", burst(mine))], a.warmup, a.rounds)
    res["model_16_requests_wall"] = wall
    res["model_16_requests"] = last
    m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
