"""Shallow fusion with a token n-gram language model, the host side (include/sonic_hip.h beside the grammar's section).

An `NGramLM` is the weighted backoff automaton lm_step_kernel (csrc/lm.hip) walks: node 0 the empty context, every other node a context of 1 .. order - 1 token
ids with a backoff link to its longest proper suffix that is a context, a backoff weight, and edges - ascending by token id - to the ids the context lists, each
with its log-probability (natural log) and the node of the longest suffix of (context . id) that is a context.  `uni[V]` is the root's log-probability of every id.
`scores` / `step` are the numpy reference of the kernel's vector and transition, operation by operation in fp32; `walk` scores a transcript; `pack` is the blob
sonic_load_tensor "lm:<id>" takes.  The builders (`from_ngrams`, `from_arpa`, `from_corpus`) are a policy of this package; the kernel contract does not depend on
them.  Needs no library and no GPU."""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

MAX_ORDER = 8
MAX_NODES = 4194304
MAX_EDGES = 16777216
HEAD = 5                # V, N, E, order, start
BOS = -1                # a context's first place may hold the sentence start (ARPA's <s>): never an edge token, so such a node is reached from `start` alone
_F = np.float32


class NGramLM:
    """A validated automaton.  ValueError names the broken rule (the library's own words); nothing is truncated."""

    def __init__(self, vocab: int, order: int, start: int, uni, node_off, bo_next, bo_w, edge_tok, edge_next, edge_w):
        self.vocab, self.order, self.start = int(vocab), int(order), int(start)
        self.uni = np.ascontiguousarray(uni, dtype=np.float32).reshape(-1)
        self.node_off = np.ascontiguousarray(node_off, dtype=np.int32).reshape(-1)
        self.bo_next = np.ascontiguousarray(bo_next, dtype=np.int32).reshape(-1)
        self.bo_w = np.ascontiguousarray(bo_w, dtype=np.float32).reshape(-1)
        self.edge_tok = np.ascontiguousarray(edge_tok, dtype=np.int32).reshape(-1)
        self.edge_next = np.ascontiguousarray(edge_next, dtype=np.int32).reshape(-1)
        self.edge_w = np.ascontiguousarray(edge_w, dtype=np.float32).reshape(-1)
        self.validate()

    @property
    def n_nodes(self) -> int:
        return len(self.bo_next)

    @property
    def n_edges(self) -> int:
        return len(self.edge_tok)

    def validate(self, vocab: Optional[int] = None) -> "NGramLM":
        """The checks the library repeats at the load, in its order and words; `vocab`: the model's vocabulary, if known"""
        V, N, E, order = self.vocab, self.n_nodes, self.n_edges, self.order
        if vocab is not None and V != int(vocab):
            raise ValueError(f"lm: the automaton's vocabulary is {V}, the model's {int(vocab)}")
        if V < 1 or len(self.uni) != V:
            raise ValueError(f"lm: uni holds {len(self.uni)} entries, the vocabulary {V}")
        if order < 1 or order > MAX_ORDER:
            raise ValueError(f"lm: order {order} is outside 1 .. {MAX_ORDER}")
        if N < 1 or N > MAX_NODES:
            raise ValueError(f"lm: {N} nodes (1 .. {MAX_NODES}; nothing is truncated)")
        if E > MAX_EDGES:
            raise ValueError(f"lm: {E} edges (0 .. {MAX_EDGES}; nothing is truncated)")
        if len(self.node_off) != N + 1 or len(self.bo_w) != N or len(self.edge_next) != E or len(self.edge_w) != E:
            raise ValueError(f"lm: the arrays do not fit {N} nodes and {E} edges")
        if self.start < 0 or self.start >= N:
            raise ValueError(f"lm: start node {self.start} (0 .. {N - 1})")
        if not np.isfinite(self.uni).all():
            raise ValueError(f"lm: uni[{int(np.argmin(np.isfinite(self.uni)))}] is not finite")
        off = self.node_off.astype(np.int64)
        if off[0] != 0:
            raise ValueError(f"lm: node_off[0] is {int(off[0])}, not 0")
        if off[N] != E:
            raise ValueError(f"lm: node_off[{N}] is {int(off[N])}, not the edge count {E}")
        d = np.diff(off)
        if (d < 0).any():
            raise ValueError(f"lm: node_off is not monotone at node {int(np.argmax(d < 0))}")
        if self.bo_next[0] != -1:
            raise ValueError(f"lm: bo_next[0] is {int(self.bo_next[0])}, not -1 (node 0 is the root)")
        bad = (self.bo_next[1:] < 0) | (self.bo_next[1:] >= np.arange(1, N))
        if bad.any():
            n = int(np.argmax(bad)) + 1
            raise ValueError(f"lm: bo_next[{n}] is {int(self.bo_next[n])} (0 .. {n - 1}: nodes are numbered by context length)")
        depth = np.zeros(N, np.int32)
        for n in range(1, N):                                     # (bo_next[n] < n: one ascending pass)
            depth[n] = depth[self.bo_next[n]] + 1
            if depth[n] > order - 1:
                raise ValueError(f"lm: the backoff chain of node {n} has {int(depth[n])} links (at most order - 1 = {order - 1})")
        if not np.isfinite(self.bo_w).all():
            raise ValueError(f"lm: bo_w[{int(np.argmin(np.isfinite(self.bo_w)))}] is not finite")
        tok = self.edge_tok
        if ((tok < 0) | (tok >= V)).any():
            raise ValueError(f"lm: token id {int(tok[(tok < 0) | (tok >= V)][0])} is out of vocabulary ({V})")
        inner = np.ones(E, bool)
        inner[off[:-1][off[:-1] < E]] = False                     # the first edge of every node has no predecessor to ascend from
        if E > 1 and (inner[1:] & (tok[1:] <= tok[:-1])).any():
            k = int(np.argmax(inner[1:] & (tok[1:] <= tok[:-1]))) + 1
            raise ValueError(f"lm: the edges of node {int(np.searchsorted(off, k, side='right') - 1)} are not sorted and unique by token id")
        nxt = self.edge_next
        if ((nxt < 0) | (nxt >= N)).any():
            raise ValueError(f"lm: an edge leads to node {int(nxt[(nxt < 0) | (nxt >= N)][0])} (0 .. {N - 1})")
        if not np.isfinite(self.edge_w).all():
            raise ValueError(f"lm: edge_w[{int(np.argmin(np.isfinite(self.edge_w)))}] is not finite")
        r = slice(0, int(off[1]))
        same = self.edge_w[r].view(np.int32) == self.uni[tok[r]].view(np.int32)
        if not same.all():
            k = int(np.argmin(same))
            raise ValueError(f"lm: root edge {k} (token {int(tok[k])}) does not carry the bits of uni[{int(tok[k])}]")
        return self

    # ---- the kernel's reference
    def chain(self, state: int) -> Tuple[List[int], List[np.float32]]:
        """the nodes c_0 = state .. c_k = 0 and the weights A_0 = +0 .. A_k gathered along them, fp32 adds in that order"""
        c, A = [int(state)], [_F(0.0)]
        while c[-1] != 0:
            A.append(_F(A[-1] + self.bo_w[c[-1]]))
            c.append(int(self.bo_next[c[-1]]))
        return c, A

    def scores(self, state: int, weight: float = 1.0) -> np.ndarray:
        """the [V] fp32 vector a row at `state` adds to its scores: weight * (A_k + uni) everywhere, then the chain's levels from the shortest context to the longest
        write weight * (A_j + edge_w) at their ids - the longest context that lists an id wins"""
        lam = _F(weight)
        c, A = self.chain(state)
        k = len(c) - 1
        add = (lam * (A[k] + self.uni)).astype(np.float32)
        for j in range(k - 1, -1, -1):
            a, b = int(self.node_off[c[j]]), int(self.node_off[c[j] + 1])
            add[self.edge_tok[a:b]] = lam * (A[j] + self.edge_w[a:b])
        return add

    def _find(self, n: int, tok: int) -> int:
        a, b = int(self.node_off[n]), int(self.node_off[n + 1])
        k = a + int(np.searchsorted(self.edge_tok[a:b], tok))
        return k if k < b and self.edge_tok[k] == tok else -1

    def step(self, state: int, tok: int) -> int:
        """the state behind an emitted token: the edge's `next` at the first node of the chain that lists it; the root if none does or the id is outside [0, V)"""
        tok, n = int(tok), int(state)
        if tok < 0 or tok >= self.vocab:
            return 0
        while True:
            k = self._find(n, tok)
            if k >= 0:
                return int(self.edge_next[k])
            if n == 0:
                return 0
            n = int(self.bo_next[n])

    def logp(self, state: int, tok: int) -> float:
        """the unweighted score of one id at `state` (scores(state)[tok], without the vector)"""
        c, A = self.chain(state)
        for j in range(len(c) - 1):
            k = self._find(c[j], int(tok))
            if k >= 0:
                return float(_F(A[j] + self.edge_w[k]))
        return float(_F(A[-1] + self.uni[int(tok)]))

    def walk(self, ids: Iterable[int], state: Optional[int] = None) -> Tuple[int, float]:
        """(the state behind `ids`, the sum of their log-probabilities), from `state` (default: the start node); ids outside the vocabulary count 0 and lead to the root"""
        n, total = self.start if state is None else int(state), 0.0
        for t in ids:
            t = int(t)
            if 0 <= t < self.vocab:
                total += self.logp(n, t)
            n = self.step(n, t)
        return n, total

    def pack(self) -> np.ndarray:
        """[V | N | E | order | start | uni[V] | node_off[N + 1] | bo_next[N] | bo_w[N] | edge_tok[E] | edge_next[E] | edge_w[E]] as int32 words (floats as their bits)"""
        head = np.array([self.vocab, self.n_nodes, self.n_edges, self.order, self.start], np.int32)
        return np.concatenate([head, self.uni.view(np.int32), self.node_off, self.bo_next, self.bo_w.view(np.int32),
                               self.edge_tok, self.edge_next, self.edge_w.view(np.int32)]).astype(np.int32)

    @classmethod
    def unpack(cls, words) -> "NGramLM":
        w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
        if len(w) < HEAD:
            raise ValueError(f"lm: {len(w)} words do not hold the header [V | N | E | order | start]")
        V, N, E, order, start = (int(x) for x in w[:HEAD])
        if V < 1 or N < 1 or E < 0 or len(w) != HEAD + V + (N + 1) + 2 * N + 3 * E:
            raise ValueError(f"lm: {len(w)} words, the header (V {V}, N {N}, E {E}) asks for {HEAD + V + (N + 1) + 2 * N + 3 * E}")
        parts, at = [], HEAD
        for n in (V, N + 1, N, N, E, E, E):
            parts.append(w[at:at + n]); at += n
        return cls(V, order, start, parts[0].view(np.float32), parts[1], parts[2], parts[3].view(np.float32), parts[4], parts[5], parts[6].view(np.float32))

    # ---- builders
    @classmethod
    def from_ngrams(cls, vocab: int, ngrams: Mapping[Tuple[int, ...], Tuple[float, float]], floor: float = -20.0) -> "NGramLM":
        """The backoff model `ngrams` states: {ids: (log-probability of the last id behind the others, backoff weight of the ids as a context)}, natural logs, rounded once
        to fp32.  A context's first id may be BOS (-1, the sentence start): decoding then starts at the node of (BOS,).  Ids without a unigram get `floor`.  A node is made
        for every context that has continuations or a backoff weight other than 0.  ValueError for an n-gram whose prefix is missing, an id out of vocabulary, a broken cap."""
        V = int(vocab)
        grams = {tuple(int(t) for t in k): (float(v[0]), float(v[1])) for k, v in ngrams.items()}
        order = max([len(k) for k in grams] + [1])
        if order > MAX_ORDER:
            raise ValueError(f"lm: order {order} is outside 1 .. {MAX_ORDER}")
        for k in grams:
            if not k:
                raise ValueError("lm: an empty n-gram")
            if any((t < 0 or t >= V) and not (t == BOS and i == 0) for i, t in enumerate(k)):
                raise ValueError(f"lm: n-gram {k} holds an id out of vocabulary ({V})")
            if len(k) > 1 and k[:-1] not in grams and k[:-1] != (BOS,):
                raise ValueError(f"lm: n-gram {k} is listed, its prefix {k[:-1]} is not")
        ctx = {()}
        for k, (_, bo) in grams.items():
            if len(k) > 1:
                ctx.add(k[:-1])
            if bo != 0.0 and len(k) < order:
                ctx.add(k)
        nodes = sorted(ctx, key=lambda c: (len(c), c))
        if len(nodes) > MAX_NODES:
            raise ValueError(f"lm: {len(nodes)} nodes (1 .. {MAX_NODES}; nothing is truncated)")
        index = {c: i for i, c in enumerate(nodes)}

        def suffix(c: Tuple[int, ...], proper: bool) -> int:      # the longest (proper) suffix of c that is a context
            for s in range(1 if proper else 0, len(c) + 1):
                if c[s:] in index:
                    return index[c[s:]]
            return 0

        uni = np.full(V, floor, np.float64)
        for k, (lp, _) in grams.items():
            if len(k) == 1 and k[0] >= 0:
                uni[k[0]] = lp
        uni = uni.astype(np.float32)
        by_ctx: Dict[Tuple[int, ...], List[Tuple[int, float]]] = {c: [] for c in nodes}
        for k, (lp, _) in grams.items():
            if len(k) > 1:
                by_ctx[k[:-1]].append((k[-1], lp))
        by_ctx[()] = [(c[0], float(uni[c[0]])) for c in nodes if len(c) == 1 and c[0] >= 0]      # root edges: the transition alone, with uni's bits
        off, tok, nxt, w, bo_next, bo_w = [0], [], [], [], [], []
        for c in nodes:
            for t, lp in sorted(by_ctx[c]):
                tok.append(t); w.append(lp); nxt.append(suffix((c + (t,))[-(order - 1):] if order > 1 else (), False))
            off.append(len(tok))
            bo_next.append(-1 if not c else suffix(c, True))
            bo_w.append(grams.get(c, (0.0, 0.0))[1] if c else 0.0)
        if len(tok) > MAX_EDGES:
            raise ValueError(f"lm: {len(tok)} edges (0 .. {MAX_EDGES}; nothing is truncated)")
        return cls(V, order, index.get((BOS,), 0), uni, off, bo_next, np.array(bo_w, np.float64).astype(np.float32), tok, nxt, np.array(w, np.float64).astype(np.float32))

    @classmethod
    def from_arpa(cls, text_or_path: str, vocab: int, token_id: Union[None, Mapping[str, int], Callable[[str], Optional[int]]] = None, eos_ids: Sequence[int] = (),
                  floor: float = -20.0) -> "NGramLM":
        """ARPA as KenLM writes it, over token strings (`token_id`: a mapping or a callable, string -> id) or decimal ids (token_id=None).  log10 becomes ln, rounded once
        to fp32.  <s> is the sentence start (BOS), </s> maps to every id of `eos_ids`, <unk> is dropped; ids the file lacks get `floor`.  ValueError for an unknown
        token and for an n-gram whose prefix context is missing."""
        text = text_or_path
        if "\n" not in text and os.path.exists(text):
            with open(text, "r", encoding="utf-8") as f:
                text = f.read()
        look = (lambda s: int(s) if s.lstrip("-").isdigit() else None) if token_id is None else (token_id.get if hasattr(token_id, "get") else token_id)
        ln10 = math.log(10.0)
        grams: Dict[Tuple[int, ...], Tuple[float, float]] = {}
        n = 0
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:-len("-grams:")])
                continue
            if n == 0:
                continue
            f = line.split()
            if len(f) not in (n + 1, n + 2):
                raise ValueError(f"lm: ARPA line {line!r} does not hold a {n}-gram")
            lp, words, bo = float(f[0]) * ln10, f[1:1 + n], (float(f[1 + n]) * ln10 if len(f) == n + 2 else 0.0)
            if "<unk>" in words or "<s>" in words[1:]:      # (the unigram <s> stays: its backoff weight is the start node's)
                continue
            keys: List[Tuple[int, ...]] = [()]
            for i, s in enumerate(words):
                if s == "<s>":
                    ids = [BOS]
                elif s == "</s>":
                    ids = [int(e) for e in eos_ids]
                else:
                    t = look(s)
                    if t is None:
                        raise ValueError(f"lm: ARPA token {s!r} has no id")
                    ids = [int(t)]
                keys = [k + (t,) for k in keys for t in ids]
            for k in keys:
                grams[k] = (lp, bo)
        if not grams:
            raise ValueError("lm: the ARPA text holds no n-grams")
        return cls.from_ngrams(vocab, grams, floor=floor)

    @classmethod
    def from_corpus(cls, token_sequences: Iterable[Sequence[int]], vocab: int, order: int = 3, discount: float = 0.75, eos_ids: Sequence[int] = ()) -> "NGramLM":
        """Interpolated absolute discounting over the counts of `token_sequences` (each closed by eos_ids[0] when given), stated in backoff form: a listed n-gram carries
        its whole interpolated probability, a context's backoff weight the mass its discounts freed.  The unigram level is interpolated with the uniform distribution
        over `vocab`, so every state's distribution sums to 1."""
        V, D = int(vocab), float(discount)
        if order < 1 or order > MAX_ORDER:
            raise ValueError(f"lm: order {order} is outside 1 .. {MAX_ORDER}")
        if not 0.0 < D < 1.0:
            raise ValueError(f"lm: discount {discount} is outside (0, 1)")
        counts: List[Dict[Tuple[int, ...], Dict[int, int]]] = [dict() for _ in range(order)]      # [context length][context][id]
        for seq in token_sequences:
            s = [int(t) for t in seq] + ([int(eos_ids[0])] if len(eos_ids) else [])
            if any(t < 0 or t >= V for t in s):
                raise ValueError(f"lm: a token sequence holds an id out of vocabulary ({V})")
            for i, t in enumerate(s):
                for L in range(min(order - 1, i) + 1):
                    d = counts[L].setdefault(tuple(s[i - L:i]), {})
                    d[t] = d.get(t, 0) + 1
        root = counts[0].get((), {})
        total = sum(root.values())
        if total == 0:
            raise ValueError("lm: the corpus holds no tokens")
        g0 = D * len(root) / total
        p_uni = np.full(V, g0 / V, np.float64)
        for t, c in root.items():
            p_uni[t] += (c - D) / total
        prob: Dict[Tuple[int, ...], float] = {}
        grams: Dict[Tuple[int, ...], Tuple[float, float]] = {}

        def p(ctx: Tuple[int, ...], t: int) -> float:            # the interpolated probability of t behind ctx (a context with counts, or shorter ones)
            if not ctx:
                return float(p_uni[t])
            d = counts[len(ctx)].get(ctx)
            if d is None:
                return p(ctx[1:], t)
            key = ctx + (t,)
            if key not in prob:
                c = sum(d.values())
                prob[key] = max(d.get(t, 0) - D, 0.0) / c + D * len(d) / c * p(ctx[1:], t)
            return prob[key]

        for t in range(V):
            grams[(t,)] = (math.log(p_uni[t]), 0.0)
        for L in range(1, order):
            for ctx, d in counts[L].items():
                c = sum(d.values())
                lp_ctx, _ = grams[ctx]
                grams[ctx] = (lp_ctx, math.log(D * len(d) / c))
                for t in d:
                    grams[ctx + (t,)] = (math.log(p(ctx, t)), 0.0)
        return cls.from_ngrams(V, grams)


def load(lm, vocab: int, eos_ids: Sequence[int] = (), token_id=None) -> NGramLM:
    """ASRModel's `lm=` argument -> an NGramLM for a model of `vocab` ids: the automaton itself, or the path of an ARPA file"""
    if isinstance(lm, NGramLM):
        return lm.validate(vocab)
    if isinstance(lm, (str, os.PathLike)):
        return NGramLM.from_arpa(os.fspath(lm), vocab, token_id=token_id, eos_ids=eos_ids).validate(vocab)
    raise ValueError("lm= takes an ngram.NGramLM or the path of an ARPA file")


def check_weight(lm_weight) -> float:
    """ASRModel's `lm_weight` argument -> the fp32 weight, or ValueError by name"""
    try:
        w = float(np.float32(lm_weight))
    except (TypeError, ValueError):
        raise ValueError(f"lm_weight must be a finite number >= 0 (got {lm_weight!r})") from None
    if isinstance(lm_weight, bool) or not math.isfinite(w) or w < 0.0:
        raise ValueError(f"lm_weight must be a finite number >= 0 (got {lm_weight!r})")
    return w
