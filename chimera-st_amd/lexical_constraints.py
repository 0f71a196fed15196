"""Lexical constraints of a hypothesis ("these phrases must appear in the translation") — the host form of the state machines that
fairseq's LexicallyConstrainedBeamSearch keeps per beam item (search.py:210-523 with token_generation_constraints.py), written from
their behaviour; the device form is the table / state pair of cst_lex_init and cst_beam_step_lex (include/cst.h).

A sentence's constraints are a list of token sequences.  A batch of them travels PACKED, int64 [bsz, W], zero-padded:
    [count, tokens of constraint 0, 0, tokens of constraint 1, 0, ...]
(0 is the terminator, so it cannot be a constraint token; neither can pad or eos: pad is never selected and eos ends a hypothesis.)

Two representations, both immutable values with the same interface — advance(token) -> state, next_tokens() -> sorted list, bank,
finished, num_distinct:
  OrderedState     the constraints must appear in the given order (anything may stand between them): the state is an index into the
                   concatenated constraints, -1 at the root;
  UnorderedState   in any order: a position in a trie of the constraints plus, per trie node, how often it was generated and how
                   often completed.
`bank` counts the constraint tokens a hypothesis has generated, `num_distinct` the DISTINCT constraint tokens of the sentence: the two
the search's sort key is made of.  The quirks of the reference are kept (see the methods): they decide hypotheses."""
from typing import List, Sequence

import torch

ORDERED, UNORDERED = "ordered", "unordered"
REPRESENTATIONS = {ORDERED: 1, UNORDERED: 2}  # cst_lex_desc.representation
MAX_TOKENS = 32       # constraint tokens per sentence the device engine holds
MAX_NEXT_TOKENS = 16  # next tokens of any one state it lists


def pack_constraints(batch_constraints: Sequence[Sequence[Sequence[int]]], pad=None, eos=None) -> torch.Tensor:
    """List over sentences of lists of token sequences (lists or 1-D tensors) -> the packed int64 [bsz, W],
    W = max over sentences of 1 + tokens + count (1 for a batch without constraints)."""
    rows = []
    for sent in batch_constraints:
        row = [len(sent)]
        for c in sent:
            c = [int(t) for t in (c.tolist() if torch.is_tensor(c) else c)]
            if not c:
                raise ValueError("an empty constraint")
            for t in c:
                if t == 0 or (pad is not None and t == pad) or (eos is not None and t == eos) or t < 0:
                    raise ValueError("constraint token %d: 0 (the terminator of the packed layout), pad, eos and negative ids cannot be "
                                     "constraint tokens" % t)
            row += c + [0]
        rows.append(row)
    width = max([len(r) for r in rows] + [1])
    out = torch.zeros(len(rows), width, dtype=torch.long)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.long)
    return out


def unpack_constraints(row) -> List[List[int]]:
    """One row of the packed tensor -> its list of token lists."""
    row = [int(t) for t in (row.tolist() if torch.is_tensor(row) else row)]
    out, at = [], 1
    for _ in range(row[0]):
        end = row.index(0, at)
        out.append(row[at:end])
        at = end + 1
    return out


class OrderedState:
    __slots__ = ("seq", "ends", "num_distinct", "state")

    def __init__(self, seq, ends, num_distinct, state=-1):
        self.seq, self.ends, self.num_distinct, self.state = seq, ends, num_distinct, state

    @classmethod
    def create(cls, row):
        cons = unpack_constraints(row)
        seq = [t for c in cons for t in c]
        ends = [i == len(c) - 1 for c in cons for i in range(len(c))]
        return cls(seq, ends, len(set(seq)), -1)

    bank = property(lambda self: self.state + 1)
    finished = property(lambda self: self.state + 1 == len(self.seq))

    def next_tokens(self):
        """The first token of all (once the state is past it — `state > 0`, so not in state 0), and the token that advances."""
        out = set()
        if self.state > 0:
            out.add(self.seq[0])
        if not self.finished:
            out.add(self.seq[self.state + 1])
        return sorted(out)

    def advance(self, token):
        token, s = int(token), self.state
        if self.finished:
            n = s
        elif self.seq[s + 1] == token:
            n = s + 1
        elif self.ends[s]:  # between two constraints anything goes; at the root this reads ends[-1], the LAST entry, which is always
            n = s           # True: a token that does not start the constraints keeps the root
        elif token == self.seq[0]:
            n = 0
        else:
            n = -1
        return OrderedState(self.seq, self.ends, self.num_distinct, n)


class Trie:
    """Node 0 is the root; per node its token, parent, terminal count (constraints ending here), num_constraints (constraints ending
    here or below) and children {token: node}."""

    def __init__(self, constraints):
        self.token, self.parent, self.terminal, self.num_constraints, self.children = [-1], [-1], [0], [0], [{}]
        for c in constraints:
            node = 0
            for t in c:
                nxt = self.children[node].get(t)
                if nxt is None:
                    nxt = len(self.token)
                    self.token.append(t), self.parent.append(node), self.terminal.append(0), self.num_constraints.append(0)
                    self.children.append({})
                    self.children[node][t] = nxt
                node = nxt
            self.terminal[node] += 1
            while node >= 0:
                self.num_constraints[node] += 1
                node = self.parent[node]
        self.num_distinct = len(set(self.token[1:]))


class UnorderedState:
    __slots__ = ("trie", "node", "generated", "completed")

    def __init__(self, trie, node=0, generated=None, completed=None):
        self.trie, self.node = trie, node
        self.generated = dict(generated or {})
        self.completed = dict(completed or {})
        if node != 0:
            self.generated[node] = self.generated.get(node, 0) + 1

    @classmethod
    def create(cls, row):
        return cls(Trie(unpack_constraints(row)))

    num_distinct = property(lambda self: self.trie.num_distinct)
    bank = property(lambda self: sum(self.generated.values()))

    @property
    def finished(self):
        t = self.trie
        pending = 1 if t.terminal[self.node] and self.completed.get(self.node, 0) < t.terminal[self.node] else 0
        return t.num_constraints[0] - (sum(self.completed.values()) + pending) == 0

    def next_tokens(self):
        out = set(self.trie.children[0])
        if self.node != 0:
            out |= set(self.trie.children[self.node])
        return sorted(out)

    def _open(self, child):
        """The edge to `child` can be taken: fewer passes through it than constraints behind it."""
        return child is not None and self.generated.get(child, 0) < self.trie.num_constraints[child]

    def advance(self, token):
        token, t = int(token), self.trie
        child = t.children[self.node].get(token)
        if self._open(child):
            return UnorderedState(t, child, self.generated, self.completed)
        # fall off the trie: restart at the root (taking the token's edge there if it is open), and settle the path that is left behind —
        # the deepest unfinished terminal on it is marked completed; the nodes below it are un-generated
        child = t.children[0].get(token)
        nxt = UnorderedState(t, child if self._open(child) else 0, self.generated, self.completed)
        node = self.node
        while node != 0:
            if t.terminal[node] and self.completed.get(node, 0) < t.terminal[node]:
                nxt.completed[node] = nxt.completed.get(node, 0) + 1
                break
            nxt.generated[node] = nxt.generated.get(node, 0) - 1
            node = t.parent[node]
        return nxt


def create_state(representation, row):
    if representation == ORDERED:
        return OrderedState.create(row)
    if representation == UNORDERED:
        return UnorderedState.create(row)
    raise ValueError("constraint representation %r (ordered | unordered)" % (representation,))


def device_limits_ok(packed) -> bool:
    """The limits of cst_lex_init: at most MAX_TOKENS constraint tokens per sentence, at most MAX_NEXT_TOKENS next tokens in any state
    (an unordered state lists the root's children and its node's)."""
    for row in packed.tolist():
        cons = unpack_constraints(row)
        if sum(len(c) for c in cons) > MAX_TOKENS:
            return False
        trie = Trie(cons)
        if any(len(set(trie.children[0]) | set(ch)) > MAX_NEXT_TOKENS for ch in trie.children):
            return False
    return True
