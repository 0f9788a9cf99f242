"""The three per-request stages on ONE handle (options request_bias, sampling and grammar; csrc/engine_generation.cpp lists them once): every option has an
invariance test of its own, this one has a batch in which request 0 carries a bias table, request 1 a temperature and a seed, request 2 a grammar and request 3
all three.  The same ids and the same log-probability bits on every path; a refused batch leaves nothing behind in any stage; a slot inherits the three options;
every grammar reference is handed back by the last fetch."""
import numpy as np
import pytest

from gpu_common import prompt_for, same_bits
from sonicscribe_amd import synth
from sonicscribe_amd.reqbias import RequestBias
from test_gpu_grammar import D, grammar_a, grammar_b, make  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(got, want, tag):
    for r in range(len(want[0])):
        assert np.array_equal(got[0][r], want[0][r]) and same_bits(got[1][r], want[1][r]), (tag, r, got[0][r].tolist(), want[0][r].tolist())


def test_three_stages_together():
    from sonicscribe_amd.engine import SonicError
    segs = [synth.synth_pcm(700 + i, n) for i, n in enumerate((48000, 200000, 80000, 64000))]
    prompts = [prompt_for(D, len(s)) for s in segs]
    budgets = [9, 12, 11, 7]
    ga, gb = grammar_a(), grammar_b()
    e = make(max_batch=8)                                    # token_logprobs and grammar on, max_ctx 1024
    e.set_option("request_bias", 1)
    e.set_option("sampling", 1)
    slot = pre = None
    try:
        da, db = e.grammar_create(ga), e.grammar_create(gb)
        run = lambda h, **kw: (lambda o: (o[0], o[2]))(h.transcribe_batch(segs, prompts, budgets, want_logprobs=True, **kw))
        plain = run(e)                                       # the handle's first run: fresh, nothing staged
        # request 0's table: one -inf entry (its free first id, so the runner-up `a` comes first) and one length-2 entry that binds behind `a`
        ban = RequestBias(bad_words_ids=[[int(plain[0][0][0])]])
        a = int(e.transcribe_batch(segs[:1], prompts[:1], [1], request_bias=[ban])[0][0][0])
        assert a != int(plain[0][0][0])
        t0 = RequestBias([[[a, 210], 1000.0]], bad_words_ids=[[int(plain[0][0][0])]])
        t3 = RequestBias([[[205, 412], 1000.0]], bad_words_ids=[[411]])      # inside grammar A's choices: 205 then 412 is preferred, 411 is banned
        kw = dict(request_bias=[t0, None, None, t3], request_sampling=[None, (0.7, 20260128), None, (0.7, 77)], request_grammar=[None, None, db, da])

        # (a) eager batch, hipGraph batch, a slot, and (below) prefill on a slot + splice in permuted row order + fetch_rows
        o = e.transcribe_batch(segs, prompts, budgets, want_logits=True, want_logprobs=True, **kw)
        want = (o[0], o[2])
        print("under the three stages", [i.tolist() for i in want[0]], "free", [i.tolist() for i in plain[0]])
        assert want[0][0][:2].tolist() == [a, 210], "request 0's table binds"
        assert not np.array_equal(want[0][1], plain[0][1]), "request 1 samples"
        assert gb.walk(want[0][2]) in ("accepted", "incomplete") and ga.walk(want[0][3]) in ("accepted", "incomplete"), "requests 2 and 3 follow their grammars"
        assert 411 not in want[0][3].tolist()
        _same(run(e, **kw), want, "graph")
        # (c) a slot created after the options were set has them: the three setters accept its batch, and the owner accepts its rows
        slot = e.slot()
        assert slot.token_logprobs and slot.request_bias and slot.sampling and slot.grammar
        _same(run(slot, **kw), want, "slot")

        # (b) all three stages staged for 4 requests, a batch of 3: refused by count, and nothing of any stage reaches the next batch
        e.set_request_bias(kw["request_bias"]); e.set_request_sampling(kw["request_sampling"]); e.set_request_grammar(kw["request_grammar"])
        with pytest.raises(SonicError, match="for 4 requests, the batch has 3"):
            e.transcribe_batch(segs[:3], prompts[:3], budgets[:3])
        _same(run(e), plain, "after the refused batch")

        pre = e.slot()
        e.service_begin()
        try:
            pre.stage_pcm(segs); pre.prefill(prompts, budgets, **kw)
            rows = {5: 0, 2: 1, 7: 2, 0: 3}                  # loop row -> request
            seq = e.splice_rows(pre, [rows[r] for r in rows], list(rows))
            got = {}
            for _ in range(300):
                fin, nn, s_, _ = e.service_step(1, 8)
                done = [r for r in rows if r not in got and s_ > seq and fin[r]]
                if done:
                    x, y = e.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                    got.update({r: (xi, yi) for r, xi, yi in zip(done, x, y)})
                if len(got) == 4:
                    break
            assert len(got) == 4
            # (d) straight after the last fetch, with every handle still alive: each row, staged request and finished batch has let go of its grammar
            da.close(); db.close()
            by_req = sorted(rows, key=lambda r: rows[r])
            _same(([got[r][0] for r in by_req], [got[r][1] for r in by_req]), want, "spliced")
        finally:
            e.service_end()
    finally:
        for h in (pre, slot):
            if h is not None:
                h.close()
        e.close()
