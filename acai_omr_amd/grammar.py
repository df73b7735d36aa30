"""Token automata for grammar-constrained decoding and the well-formedness reward (an extension: the reference knows no grammar).

A `TokenAutomaton` is a table `next[state][token]` (int16): a non-negative entry is the state after emitting that token, a negative entry
forbids the token in that state.  The same table serves two kernels:

  * the selection launch of a decode step (acai_decode_grammar_step and its sampled / slot forms, DecodeEngine.greedy(grammar=) ...) treats
    the forbidden tokens of a row's state as -inf logits and advances the state;
  * acai_grammar_scan (ops.grammar_scan) walks finished rollouts, counts the forbidden transitions and reports whether a row ended with an
    allowed <eos>: the inputs of train.grpo.calc_wellformedness.

No LMX grammar ships with the package: the linearizer that defines it is not part of it, and a grammar written from memory would forbid
valid music without anyone noticing.  What ships is the mechanism and two builders: `from_corpus` learns the automaton from target sequences
(every user of the training loops has them), `from_transitions` takes explicit rules.  What a learned automaton does to the output of a
trained checkpoint has not been measured.

There is no accept set: a sequence may end in state s exactly when next[s][<eos>] >= 0."""
import torch

MAX_STATES = 32767


class TokenAutomaton:
    """next: int16 [S][V]; start: the state after <bos>; resync: int16 [V], the state taken after a token that was not allowed (the scan goes
    on counting from it; the decode step uses it when a state allows no token at all).  Build one with from_transitions / permissive /
    from_corpus: the constructor does not validate."""

    def __init__(self, next, start, resync, pad_idx, bos_idx, eos_idx):
        self.next, self.start, self.resync = next, int(start), resync
        self.pad_idx, self.bos_idx, self.eos_idx = int(pad_idx), int(bos_idx), int(eos_idx)

    @property
    def states(self):
        return int(self.next.shape[0])

    @property
    def vocab_size(self):
        return int(self.next.shape[1])

    @property
    def device(self):
        return self.next.device

    # ---- builders ------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_transitions(cls, next, start, resync=None, *, pad_idx, bos_idx, eos_idx):
        """Validated automaton from an explicit table (anything torch.as_tensor takes, integer, [S][V]).  ValueError for: a shape or an entry
        out of range (1 <= S <= 32767, entries < S, 0 <= start < S, resync [V] in [0, S)), a state that allows <bos> or <pad>, and a state
        reachable from `start` that allows no token.  resync defaults to next[start][k] where that is allowed, else start."""
        nxt = torch.as_tensor(next)
        if nxt.dim() != 2 or nxt.dtype.is_floating_point or nxt.dtype == torch.bool:
            raise ValueError(f"next must be an integer table [states][vocabulary], got shape {tuple(nxt.shape)} dtype {nxt.dtype}")
        nxt = nxt.detach().cpu().long()
        S, V = nxt.shape
        if not 1 <= S <= MAX_STATES or V < 1:
            raise ValueError(f"next has {S} states over {V} tokens: needs 1 <= states <= {MAX_STATES} and a non-empty vocabulary")
        if int(nxt.max()) >= S:
            raise ValueError(f"next holds the state {int(nxt.max())}, outside [0, {S})")
        if int(nxt.min()) < -32768:
            raise ValueError(f"next holds {int(nxt.min())}, which does not fit 16 bits")
        start = int(start)
        if not 0 <= start < S:
            raise ValueError(f"start {start} outside [0, {S})")
        for name, k in (("pad_idx", pad_idx), ("bos_idx", bos_idx), ("eos_idx", eos_idx)):
            if not 0 <= int(k) < V:
                raise ValueError(f"{name} {k} outside [0, {V})")
        for name, k in (("<bos>", bos_idx), ("<pad>", pad_idx)):
            bad = (nxt[:, int(k)] >= 0).nonzero()
            if bad.numel():
                raise ValueError(f"state {int(bad[0])} allows {name}: an automaton never allows <bos> or <pad>")
        # reachability over the distinct (state, successor) edges, breadth first
        src, tok = (nxt >= 0).nonzero(as_tuple=True)
        edges = torch.unique(src * S + nxt[src, tok])
        edst = (edges % S).tolist()
        first_edge = torch.searchsorted(edges, torch.arange(S + 1) * S).tolist()
        seen = [False] * S
        seen[start] = True
        queue = [start]
        while queue:
            s = queue.pop()
            if first_edge[s] == first_edge[s + 1]:
                raise ValueError(f"state {s} is reachable from start {start} and allows no token")
            for n in edst[first_edge[s]:first_edge[s + 1]]:
                if not seen[n]:
                    seen[n] = True
                    queue.append(n)
        if resync is None:
            row = nxt[start]
            rs = torch.where(row >= 0, row, torch.full_like(row, start))
        else:
            rs = torch.as_tensor(resync)
            if rs.shape != (V,) or rs.dtype.is_floating_point or rs.dtype == torch.bool:
                raise ValueError(f"resync must be an integer vector [{V}], got shape {tuple(rs.shape)} dtype {rs.dtype}")
            rs = rs.detach().cpu().long()
            if int(rs.min()) < 0 or int(rs.max()) >= S:
                raise ValueError(f"resync holds a state outside [0, {S})")
        return cls(nxt.to(torch.int16).contiguous(), start, rs.to(torch.int16).contiguous(), pad_idx, bos_idx, eos_idx)

    @classmethod
    def permissive(cls, V, *, pad_idx, bos_idx, eos_idx):
        """One state in which every token but <bos> and <pad> is allowed: constrained decoding under it picks what unconstrained decoding
        picks (unless the model prefers one of those two), with log-probs renormalised over the other tokens."""
        nxt = torch.zeros(1, int(V), dtype=torch.long)
        nxt[0, int(bos_idx)] = nxt[0, int(pad_idx)] = -1
        return cls.from_transitions(nxt, 0, pad_idx=pad_idx, bos_idx=bos_idx, eos_idx=eos_idx)

    @classmethod
    def from_corpus(cls, seqs, order=1, *, V, pad_idx, bos_idx, eos_idx):
        """The automaton of the n-grams of a corpus: seqs is a list of token sequences, each `<bos> ... <eos>` (lists or 1-D tensors).  A state
        is the context of the last `order` (1 or 2) tokens, numbered in order of first appearance; start is the context of <bos> alone; a
        transition is allowed iff it occurs in the corpus; <eos> leads to one absorbing end state that allows only <eos>.  Every corpus
        sequence is therefore accepted without a violation.  resync[k] is the first context that ends in k (the end state for <eos>, start
        for a token the corpus never holds), so that counting goes on from what was actually emitted.  ValueError for a malformed sequence
        and when more than 32767 states result."""
        order, V = int(order), int(V)
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order}")
        bos, pad, eos = int(bos_idx), int(pad_idx), int(eos_idx)
        ids = {(bos,): 0}
        trans = {}      # (state, token) -> state
        first = {}      # token -> first context ending in it
        end = None
        for n, seq in enumerate(seqs):
            toks = [int(t) for t in (seq.tolist() if torch.is_tensor(seq) else seq)]
            if len(toks) < 2 or toks[0] != bos or toks[-1] != eos:
                raise ValueError(f"corpus sequence {n} is not <bos> ... <eos>")
            ctx = (bos,)
            for p, k in enumerate(toks[1:], start=1):
                if not 0 <= k < V or k in (bos, pad) or (k == eos and p != len(toks) - 1):
                    raise ValueError(f"corpus sequence {n} holds token {k} at index {p}: outside [0, {V}), <bos>, <pad> or an inner <eos>")
                s = ids[ctx]
                if k == eos:
                    if end is None:
                        end = len(ids)
                        ids[("end",)] = end
                    trans[(s, k)] = end
                    break
                ctx = (ctx + (k,))[-order:]
                if ctx not in ids:
                    ids[ctx] = len(ids)
                    if len(ids) > MAX_STATES:
                        raise ValueError(f"the corpus has more than {MAX_STATES} contexts of order {order}")
                first.setdefault(k, ids[ctx])
                trans[(s, k)] = ids[ctx]
        if end is None:
            raise ValueError("the corpus holds no sequence")
        if len(ids) > MAX_STATES:
            raise ValueError(f"the corpus has more than {MAX_STATES} contexts of order {order}")
        nxt = torch.full((len(ids), V), -1, dtype=torch.long)
        if trans:
            idx = torch.tensor(list(trans.keys()), dtype=torch.long)
            nxt[idx[:, 0], idx[:, 1]] = torch.tensor(list(trans.values()), dtype=torch.long)
        nxt[end, eos] = end
        rs = torch.zeros(V, dtype=torch.long)
        for k, s in first.items():
            rs[k] = s
        rs[eos] = end
        return cls.from_transitions(nxt, 0, rs, pad_idx=pad, bos_idx=bos, eos_idx=eos)

    # ---- plumbing ------------------------------------------------------------------------------------------------------------------------
    def to(self, device):
        return TokenAutomaton(self.next.to(device), self.start, self.resync.to(device), self.pad_idx, self.bos_idx, self.eos_idx)

    def state_dict(self):
        """Plain tensors and ints (goes through torch.save)."""
        return {"next": self.next.detach().cpu().clone(), "resync": self.resync.detach().cpu().clone(), "start": self.start,
                "pad_idx": self.pad_idx, "bos_idx": self.bos_idx, "eos_idx": self.eos_idx}

    @classmethod
    def from_state_dict(cls, sd):
        return cls.from_transitions(sd["next"], sd["start"], sd["resync"], pad_idx=sd["pad_idx"], bos_idx=sd["bos_idx"], eos_idx=sd["eos_idx"])

    # ---- the scan, stated on the CPU --------------------------------------------------------------------------------------------------------
    def violations(self, seqs, lens=None):
        """(violations int32 [R], complete bool [R]) of the rows seqs[r][:lens[r]] - what acai_grammar_scan computes, on the CPU.  seqs: an
        integer tensor (R, ld), or a list of ragged rows (lens then defaults to their lengths); lens: int lengths (clamped to [0, ld]) or a
        bool prefix mask of seqs' shape.  Index 0 is <bos> and is not checked.  From s = start, for p = 1 .. len - 1 with k = seqs[r][p]:
        k outside [0, V) is one violation and s = start; next[s][k] < 0 is one violation and s = resync[k]; otherwise s = next[s][k].
        complete[r]: len >= 2, the last token is <eos> and its transition was allowed."""
        if not torch.is_tensor(seqs):
            rows = [torch.as_tensor(r, dtype=torch.long).reshape(-1) for r in seqs]
            if lens is None:
                lens = torch.tensor([r.numel() for r in rows], dtype=torch.long)
            pad = torch.zeros(len(rows), max([r.numel() for r in rows] + [1]), dtype=torch.long)
            for i, r in enumerate(rows):
                pad[i, :r.numel()] = r
            seqs = pad
        seqs = seqs.detach().cpu().long()
        R, ld = seqs.shape
        if lens is None:
            lens = torch.full((R,), ld, dtype=torch.long)
        lens = torch.as_tensor(lens).detach().cpu()
        lens = lens.sum(dim=-1) if lens.dtype == torch.bool else lens
        lens = lens.long().clamp(0, ld)
        nxt, rs, V = self.next.cpu().long(), self.resync.cpu().long(), self.vocab_size
        s = torch.full((R,), self.start, dtype=torch.long)
        viol = torch.zeros(R, dtype=torch.int32)
        ended = torch.zeros(R, dtype=torch.bool)
        for p in range(1, int(lens.max()) if R else 0):
            k = seqs[:, p]
            live = p < lens
            inside = (k >= 0) & (k < V)
            kc = k.clamp(0, V - 1)
            n = nxt[s, kc]
            ok = inside & (n >= 0)
            viol += (live & ~ok).int()
            s = torch.where(live, torch.where(ok, n, torch.where(inside, rs[kc], torch.full_like(s, self.start))), s)
            ended = torch.where(live & (p == lens - 1), ok & (k == self.eos_idx), ended)
        return viol, ended & (lens >= 2)

    def accepts(self, seq):
        """True when the one sequence `<bos> ... <eos>` has no violation and ends with an allowed <eos>."""
        v, c = self.violations([seq])
        return int(v[0]) == 0 and bool(c[0])
