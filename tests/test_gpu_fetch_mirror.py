"""Finished rows leave a continuous loop through a pinned mirror (csrc/engine_service.cpp service_status_kernel): the kernel behind every chunk
copies a row's ids - and its log-probability records - into pinned host memory in the chunk that finds it finished, and sonic_fetch_row / sonic_fetch_rows read
them from there with memcpy.  What must hold: whatever a row's length, wherever in a chunk it ended, whoever held the row before, with records of any width and
behind an accepted draft - the fetched arrays are those of a plain run_staged batch of the same requests, bit for bit; a row fetched before any check takes the
copy on the handle's stream; option fetch_stream = 1 (the copy commands on a stream of their own, as before the mirror) gives the same arrays.

TINY dimensions, one prefill slot, decode_chunk = 2 (a prefill leaves token 1, chunk k leaves tokens 2k and 2k + 1)."""
from dataclasses import replace

import numpy as np
import pytest

from gpu_common import bits, make_engine, prompt_for
from sonicscribe_amd import spec, synth

pytestmark = pytest.mark.gpu

DIMS = replace(spec.TINY, eos_ids=())                       # budgets alone decide where a row ends
SEGS = [synth.synth_pcm(900 + i, 16000 * (1 + i % 3)) for i in range(6)]
PROMPTS = [prompt_for(DIMS, len(s)) for s in SEGS]
LP = [("token_logprobs", 1)]


def same(a, b):
    if isinstance(a, tuple):                                # TokenScores: lp, top_logprobs, top_ids
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return b.dtype == np.float32 and a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and np.array_equal(a, b)


class Loop:
    """a continuously decoding handle and its prefill slot; `lp`: rows are fetched with their log-probability records"""

    def __init__(self, options=(), lp=False, max_batch=8, max_ctx=512):
        self.lp = lp
        self.dec = make_engine(DIMS, 0, max_batch, max_ctx, [("decode_chunk", 2)] + list(options))
        self.pre = self.dec.slot()
        self.steps = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.pre.close()
        self.dec.close()

    def plain(self, which, budgets, drafts=None):
        """the requests as one plain run_staged batch on the slot: [(ids, records or None)]"""
        self.pre.stage_pcm([SEGS[i] for i in which])
        if drafts is not None:
            self.pre.set_request_draft(drafts)
        self.pre.run_staged([PROMPTS[i] for i in which], budgets)
        got = self.pre.fetch_tokens(len(which), max(budgets), want_logprobs=self.lp)
        return list(zip(*got)) if self.lp else [(ids, None) for ids in got]

    def splice(self, which, budgets, rows, drafts=None):
        """prefill the requests on the slot and splice them into `rows`: {row: valid_after}"""
        self.pre.stage_pcm([SEGS[i] for i in which])
        self.pre.prefill([PROMPTS[i] for i in which], budgets, request_draft=drafts)
        seq = self.dec.splice_rows(self.pre, list(range(len(which))), rows)
        return {r: seq for r in rows}

    def fetch(self, rows, nn):
        got = self.dec.fetch_rows(rows, [int(nn[r]) for r in rows], want_logprobs=self.lp)
        return dict(zip(rows, zip(*got))) if self.lp else {r: (ids, None) for r, ids in zip(rows, got)}

    def drain(self, pending, top, seen=None, limit=400):
        """one chunk at a time; every row leaves in the step whose check first shows it finished.  {row: (ids, records)}; seen[row] = that check's number"""
        out = {}
        for _ in range(limit):
            fin, nn, seq, _ = self.dec.service_step(1, top)
            self.steps += 1
            done = [r for r, va in pending.items() if seq > va and fin[r]]
            if done:
                out.update(self.fetch(done, nn))
            for r in done:
                del pending[r]
                if seen is not None:
                    seen[r] = seq
            if not pending:
                return out
        raise AssertionError("rows did not finish")


def check(got, want, rows):
    """row rows[i] of the loop against request i of the plain batch"""
    for i, r in enumerate(rows):
        assert same(got[r][0], want[i][0]), (r, got[r][0], want[i][0])
        assert got[r][1] is None or same(got[r][1], want[i][1]), r


ONE_SPLICE = ([0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [6, 0, 3, 1, 4])      # requests, budgets, rows: budget 1 ends at the splice, 3 and 5 at a chunk's end, 2 and 4 inside one


def one_splice(loop):
    which, budgets, rows = ONE_SPLICE
    want = loop.plain(which, budgets)
    assert [len(w[0]) for w in want] == budgets
    loop.dec.service_begin()
    got = loop.drain(loop.splice(which, budgets, rows), 7)
    loop.dec.service_end()
    check(got, want, rows)
    return [got[r] for r in rows]


@pytest.mark.parametrize("options,lp", [((), False), (LP, True), (LP + [("top_logprobs", 2)], True)], ids=["ids", "logprobs", "top2"])
def test_budgets_one_to_five_in_one_splice(options, lp):
    """budget 1 finishes at the splice itself (its first token must arrive), the others at a chunk's end or inside a chunk; with token_logprobs the records come
    along, one float or - top_logprobs = 2 - five per token"""
    with Loop(options, lp) as loop:
        got = one_splice(loop)
        if lp and len(options) > 1:
            assert all(g[1].top_logprobs.shape == (len(g[0]), 2) for g in got)


def test_fetch_stream_gives_the_same_arrays():
    with Loop(LP, True) as a, Loop(LP + [("fetch_stream", 1)], True) as b:
        ga, gb = one_splice(a), one_splice(b)
        assert all(same(x[0], y[0]) and same(x[1], y[1]) for x, y in zip(ga, gb))
        with pytest.raises(RuntimeError):                   # the loop mirrors rows or does not, from service_begin on
            a.dec.service_begin(); a.dec.set_option("fetch_stream", 1)
        a.dec.service_end()


def test_largest_budget_the_context_admits():
    """out_cap is max_ctx, and a prompt holds at least one token: the longest row a handle admits has prompt + max_new = max_ctx"""
    with Loop(LP, True, max_batch=4, max_ctx=128) as loop:
        budget = 128 - len(PROMPTS[0])
        assert budget > 64
        with pytest.raises(RuntimeError):
            loop.pre.stage_pcm([SEGS[0]]); loop.pre.run_staged([PROMPTS[0]], [budget + 1])
        want = loop.plain([0, 3], [budget, 2])
        loop.dec.service_begin()
        got = loop.drain(loop.splice([0, 3], [budget, 2], [1, 0]), 2)
        loop.dec.service_end()
        assert len(got[1][0]) == budget
        check(got, want, [1, 0])


def test_a_short_row_after_a_long_one():
    """row 2 holds a 12-token request, is fetched, then takes a 3-token one while its neighbour keeps decoding: nothing of the first occupant appears"""
    with Loop(LP, True) as loop:
        want = loop.plain([1, 2, 4], [12, 3, 30])
        loop.dec.service_begin()
        pending = loop.splice([1, 4], [12, 30], [2, 0])
        long_one = pending.pop(0)
        got = loop.drain(pending, 3)
        pending = loop.splice([2], [3], [2])
        got2 = loop.drain(pending, 3)
        got0 = loop.drain({0: long_one}, 3)
        loop.dec.service_end()
        check(got, [want[0]], [2])
        check(got2, [want[1]], [2])
        check(got0, [want[2]], [0])
        assert len(got2[2][0]) == 3 and len(got2[2][1]) == 3


def test_two_blocks_finish_in_one_chunk():
    """block A (budget 7) is spliced in front of chunk 1, block B (budget 5) in front of chunk 2: both end with chunk 3 and leave behind the same check"""
    with Loop(LP, True) as loop:
        want_a, want_b = loop.plain([0, 1], [7, 7]), loop.plain([2, 3], [5, 5])
        loop.dec.service_begin()
        pending = loop.splice([0, 1], [7, 7], [0, 1])
        loop.dec.service_step(1, 4)
        pending.update(loop.splice([2, 3], [5, 5], [2, 3]))
        seen = {}
        got = loop.drain(pending, 4, seen)
        loop.dec.service_end()
        assert len(set(seen.values())) == 1, seen
        check(got, want_a, [0, 1])
        check(got, want_b, [2, 3])


def test_a_row_arrives_with_its_accepted_draft():
    """option draft_verify: the prefill accepts the draft, the row is spliced with several tokens, and all of them - with their records - leave through the mirror"""
    with Loop(LP + [("draft_verify", 1)], True) as loop:
        free = loop.plain([1, 2], [9, 6])
        drafts = [[int(t) for t in free[0][0][:6]], None]
        want = loop.plain([1, 2], [9, 6], drafts)
        acc = list(loop.pre.draft_accepted(2))
        assert acc[0] >= 2 and acc[1] == 0, acc             # (the draft is the model's own run: a disagreement can only come from a near tie)
        loop.dec.service_begin()
        pending = loop.splice([1, 2], [9, 6], [1, 0], drafts)
        assert list(loop.pre.draft_accepted(2)) == acc
        got = loop.drain(pending, 2)
        loop.dec.service_end()
        check(got, want, [1, 0])


def test_a_row_fetched_before_any_check_takes_the_copy():
    """the fallback: a budget-1 row is fetched right behind its splice - no chunk has run, no check has shown it, its tokens are not in the mirror - first on a
    fresh loop, then on one whose checks have seen the row free"""
    with Loop() as loop:
        want = loop.plain([0, 5, 3], [1, 1, 20])
        loop.dec.service_begin()
        loop.splice([0], [1], [2])
        assert same(loop.dec.fetch_row(2, 1), want[0][0])
        pending = loop.splice([3], [20], [0])
        for _ in range(3):
            fin, nn, seq, _ = loop.dec.service_step(1, 1)
        assert fin[2] and seq > 0
        loop.splice([5], [1], [2])
        assert same(loop.dec.fetch_rows([2], [1])[0], want[1][0])
        got = loop.drain(pending, 1)
        loop.dec.service_end()
        check(got, [want[2]], [0])
