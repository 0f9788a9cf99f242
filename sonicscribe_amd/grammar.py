"""Grammar-constrained decoding, the host side (include/sonic_hip.h beside sonic_set_request_sampling).

A `Grammar` is the deterministic token automaton the greedy kernel walks: CSR arrays `node_off[N + 1]`, `edge_tok[E]`, `edge_next[E]`, node 0 the start node,
the edges of a node sorted by token id, strictly ascending.  EOS is an ordinary edge, added where a transcript may end; there is no accept flag.  A row's state
is -1 (free: no grammar), n >= 0 (at node n) or -2 (it has left the grammar: only the EOS ids remain).  `apply` / `step` are the numpy reference of the kernel's
mask and transition, `walk` classifies a returned transcript, `prefix_allowed_tokens_fn` hands the same automaton to HF's generate().  The builders
(`from_token_sequences`, `from_phrases`) are a policy of this package; the kernel contract does not depend on them.  Needs no library and no GPU."""
from __future__ import annotations

from typing import Callable, Dict, FrozenSet, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .frontend import clean_hotwords

MAX_NODES = 65536
MAX_EDGES = 1048576
FREE, LEFT = -1, -2


class Grammar:
    """A validated automaton.  vocab / audio_token_id (optional): the checks the library repeats against its own model (an id outside [0, vocab), the audio
    placeholder).  eos_ids: the ids that end a transcript - what a row at -2 may still emit and what `walk` accepts on; the builders pass the ones they used.
    ValueError names the broken rule; nothing is truncated."""

    def __init__(self, node_off, edge_tok, edge_next, eos_ids: Iterable[int] = (), vocab: Optional[int] = None, audio_token_id: Optional[int] = None):
        off = np.ascontiguousarray(node_off, dtype=np.int64).reshape(-1)
        tok = np.ascontiguousarray(edge_tok, dtype=np.int64).reshape(-1)
        nxt = np.ascontiguousarray(edge_next, dtype=np.int64).reshape(-1)
        N, E = len(off) - 1, len(tok)
        if N < 1 or N > MAX_NODES:
            raise ValueError(f"grammar: {N} nodes (1 .. {MAX_NODES}; nothing is truncated)")
        if E < 1 or E > MAX_EDGES:
            raise ValueError(f"grammar: {E} edges (1 .. {MAX_EDGES}; nothing is truncated)")
        if len(nxt) != E:
            raise ValueError(f"grammar: edge_tok holds {E} entries, edge_next {len(nxt)}")
        if off[0] != 0:
            raise ValueError(f"grammar: node_off[0] is {off[0]}, not 0")
        if off[N] != E:
            raise ValueError(f"grammar: node_off[{N}] is {off[N]}, not the edge count {E}")
        d = np.diff(off)
        if (d < 0).any():
            raise ValueError(f"grammar: node_off is not monotone at node {int(np.argmax(d < 0))}")
        if (d == 0).any():
            raise ValueError(f"grammar: node {int(np.argmax(d == 0))} has no edge (a transcript ends through an EOS edge, never by running dry)")
        if (tok < 0).any() or (vocab is not None and (tok >= vocab).any()):
            bad = tok[(tok < 0) | (tok >= (vocab if vocab is not None else np.iinfo(np.int64).max))][0]
            raise ValueError(f"grammar: token id {int(bad)} is out of vocabulary" + (f" ({vocab})" if vocab is not None else ""))
        if audio_token_id is not None and (tok == audio_token_id).any():
            raise ValueError(f"grammar: token id {audio_token_id} is the audio placeholder, which cannot be emitted")
        if (nxt < 0).any() or (nxt >= N).any():
            raise ValueError(f"grammar: an edge leads to node {int(nxt[(nxt < 0) | (nxt >= N)][0])} (0 .. {N - 1})")
        inner = np.ones(E, bool)
        inner[off[:-1]] = False                                   # the first edge of every node has no predecessor to ascend from
        if E > 1 and (inner[1:] & (tok[1:] <= tok[:-1])).any():
            k = int(np.argmax(inner[1:] & (tok[1:] <= tok[:-1]))) + 1
            raise ValueError(f"grammar: the edges of node {int(np.searchsorted(off, k, side='right') - 1)} are not sorted and unique by token id")
        self.node_off, self.edge_tok, self.edge_next = off.astype(np.int32), tok.astype(np.int32), nxt.astype(np.int32)
        self.eos_ids: Tuple[int, ...] = tuple(int(e) for e in eos_ids)

    @property
    def n_nodes(self) -> int:
        return len(self.node_off) - 1

    @property
    def n_edges(self) -> int:
        return len(self.edge_tok)

    # ---- the kernel's reference
    def allowed(self, state: int, eos_ids: Optional[Iterable[int]] = None) -> np.ndarray:
        """the ids a row in `state` may emit, ascending (state >= 0: its node's edge tokens; -2: the EOS ids); None for a free row"""
        if state == FREE:
            return None
        if state == LEFT:
            return np.array(sorted(set(self.eos_ids if eos_ids is None else eos_ids)), np.int32)
        return self.edge_tok[self.node_off[state]:self.node_off[state + 1]]

    def apply(self, scores, state: int, eos_ids: Optional[Iterable[int]] = None) -> np.ndarray:
        """HF's PrefixConstrainedLogitsProcessor on one row: a copy of `scores` [V] with every id the state does not allow at -inf (a free row: the copy alone)"""
        s = np.array(scores, np.float32, copy=True)
        ok = self.allowed(int(state), eos_ids)
        if ok is None:
            return s
        mask = np.ones(s.shape[-1], bool)
        mask[ok[ok < s.shape[-1]]] = False
        s[..., mask] = -np.inf
        return s

    def step(self, state: int, tok: int) -> int:
        """the state behind an emitted token: the edge's `next` if the node has an edge for it, else -2; a free row stays free"""
        if state == FREE:
            return FREE
        if state < 0:
            return LEFT
        a, b = int(self.node_off[state]), int(self.node_off[state + 1])
        k = a + int(np.searchsorted(self.edge_tok[a:b], tok))
        return int(self.edge_next[k]) if k < b and self.edge_tok[k] == tok else LEFT

    def walk(self, ids: Iterable[int], eos_ids: Optional[Iterable[int]] = None) -> str:
        """"accepted": every id followed an edge and the last one is an EOS id; "incomplete": every id followed an edge, the transcript has not ended (its budget
        ran out inside the grammar); "left": an id had no edge"""
        eos = set(self.eos_ids if eos_ids is None else eos_ids)
        state, last = 0, None
        for t in ids:
            state = self.step(state, int(t))
            if state == LEFT:
                return "left"
            last = int(t)
        return "accepted" if last in eos else "incomplete"

    def prefix_allowed_tokens_fn(self, prompt_len: int, eos_ids: Optional[Iterable[int]] = None) -> Callable:
        """HF generate(prefix_allowed_tokens_fn=...): the ids allowed behind input_ids[prompt_len:], the state found by walking them from node 0"""
        def fn(batch_id, input_ids):
            state = 0
            for t in [int(x) for x in input_ids[prompt_len:]]:
                state = self.step(state, t)
            return [int(x) for x in self.allowed(state, eos_ids)]
        return fn

    # ---- builders
    @classmethod
    def _from_dfa(cls, nodes: List[Dict[int, int]], **kw) -> "Grammar":
        if len(nodes) > MAX_NODES:
            raise ValueError(f"grammar: {len(nodes)} nodes (1 .. {MAX_NODES}; nothing is truncated)")
        off, tok, nxt = [0], [], []
        for e in nodes:
            for t in sorted(e):
                tok.append(t); nxt.append(e[t])
            off.append(len(tok))
        if len(tok) > MAX_EDGES:
            raise ValueError(f"grammar: {len(tok)} edges (1 .. {MAX_EDGES}; nothing is truncated)")
        return cls(off, tok, nxt, **kw)

    @classmethod
    def from_token_sequences(cls, seqs: Sequence[Sequence[int]], eos_ids: Iterable[int], vocab: Optional[int] = None, audio_token_id: Optional[int] = None) -> "Grammar":
        """The transcripts `seqs` and nothing else: a trie whose sequence ends carry an edge per EOS id.  A sequence that is a prefix of another may end there or go
        on.  ValueError for no sequences, an empty one, one that holds an EOS id, no EOS id, a broken cap."""
        return cls._build([[tuple(int(t) for t in s) for s in seqs]], [], eos_ids, vocab, audio_token_id)

    @classmethod
    def from_phrases(cls, phrases: Sequence[str], encode: Callable[[str], Sequence[int]], eos_ids: Iterable[int], repeat: bool = False,
                     vocab: Optional[int] = None, audio_token_id: Optional[int] = None) -> "Grammar":
        """One of `phrases`, cleaned as hotwords are (frontend.clean_hotwords, without its cap): each is tokenised as it stands and with one leading space
        (`encode(text) -> ids` adds no special tokens) and may end in EOS; with repeat=True a phrase may also be followed by any phrase in its leading-space form.
        The result is determinised by subset construction.  ValueError for no usable phrase and for a broken cap."""
        cleaned = clean_hotwords(phrases, max_hotwords=max(1, len(phrases or ())))
        first, later = [], []
        for p in cleaned:
            a, b = tuple(int(t) for t in encode(p)), tuple(int(t) for t in encode(" " + p))
            for ids in (a, b):
                if ids and ids not in first:
                    first.append(ids)
            if b and b not in later:
                later.append(b)
        if not first:
            raise ValueError("grammar: no usable phrase")
        return cls._build([first], later if repeat else [], eos_ids, vocab, audio_token_id)

    @classmethod
    def _build(cls, start_sets, follow, eos_ids, vocab, audio_token_id) -> "Grammar":
        eos = sorted(set(int(e) for e in eos_ids))
        if not eos:
            raise ValueError("grammar: at least one EOS id is needed (a transcript ends through an EOS edge)")
        seqs = start_sets[0]
        if not seqs:
            raise ValueError("grammar: no token sequences")
        # the nondeterministic automaton: a trie of the start forms rooted at 0 and, for repeat, a trie of the follow forms rooted at `r`; a sequence's end is `final`
        trie: List[Dict[int, int]] = [{}]
        final = set()

        def insert(root: int, s: Tuple[int, ...]):
            if not s:
                raise ValueError("grammar: an empty token sequence")
            n = root
            for t in s:
                if t in eos:
                    raise ValueError(f"grammar: a token sequence holds the EOS id {t} (EOS edges are added by the builder)")
                if t not in trie[n]:
                    trie.append({}); trie[n][t] = len(trie) - 1
                n = trie[n][t]
            final.add(n)

        for s in seqs:
            insert(0, s)
        r = None
        if follow:
            trie.append({}); r = len(trie) - 1
            for s in follow:
                insert(r, s)
        # subset construction; a final member also stands at the follow root (the epsilon move of repeat).  A sequence end without children behaves like every other
        # one - "ended" - so all of them are the one member -1: with repeat the ends of 1 000 phrases share one node of 1 000 edges instead of owning one each
        def close(members) -> FrozenSet[int]:
            m = set(members)
            ends = m & final
            if r is not None and ends:
                m.add(r)
            leaves = {n for n in ends if not trie[n]}
            if leaves:
                m -= leaves
                m.add(-1)
            return frozenset(m)

        start = close({0})
        index = {start: 0}
        order = [start]
        nodes: List[Dict[int, int]] = []
        END = None
        i = 0
        while i < len(order):
            cur = order[i]; i += 1
            moves: Dict[int, set] = {}
            for n in cur:
                for t, m in (trie[n].items() if n >= 0 else ()):
                    moves.setdefault(t, set()).add(m)
            e: Dict[int, int] = {}
            for t, ms in moves.items():
                c = close(ms)
                if c not in index:
                    index[c] = len(order); order.append(c)
                    if len(order) > MAX_NODES:
                        raise ValueError(f"grammar: more than {MAX_NODES} nodes after determinisation (nothing is truncated)")
                e[t] = index[c]
            if -1 in cur or cur & final:
                e.update({t: END for t in eos})
            nodes.append(e)
        end = len(nodes)                                            # the node behind EOS: a finished row never steps again; EOS loops keep "every node has an edge"
        for e in nodes:
            for t in eos:
                if t in e and e[t] is END:
                    e[t] = end
        nodes.append({t: end for t in eos})
        return cls._from_dfa(nodes, eos_ids=eos, vocab=vocab, audio_token_id=audio_token_id)


class CompiledGrammar:
    """A Grammar on the device of every replica of a model (ASRModel.compile_grammar): one engine.DeviceGrammar per weight owner, shared by all of its handles and by
    any number of requests.  `grammar` is the host automaton (walk() classifies what came back).  close() raises while a staged or running request refers to it;
    the model's close() takes what is left."""

    def __init__(self, grammar: Grammar, engines: Sequence):
        self.grammar = grammar
        self._dev = {}
        try:
            for e in engines:
                if id(e.root) not in self._dev:
                    self._dev[id(e.root)] = e.grammar_create(grammar)
        except BaseException:
            self.close()
            raise

    def on(self, engine):
        """the handle that serves `engine` (its weight owner's); ValueError for an engine of another model"""
        d = self._dev.get(id(engine.root))
        if d is None or d.h is None:
            raise ValueError("this grammar was compiled for another model, or has been closed (ASRModel.compile_grammar)")
        return d

    def close(self):
        for k in list(self._dev):
            self._dev[k].close()
            del self._dev[k]

    def __bool__(self):
        return True
