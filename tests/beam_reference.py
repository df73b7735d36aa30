"""Float64 restatement of beam-search decoding (ViTOMR.cached_beam_generate / acai_decode_beam_step), on top of the oracle's decode step.

The reference decodes greedily only, so the contract is the project's own (README):
  * rows i*K + k are beam slot k of image i; every row starts from <bos> (quirk Q1: the token at index t-1 is embedded at position t);
    cum = 0 for slot 0, -inf for slots 1..K-1;
  * a live row proposes its K best tokens by raw logit (lower index first on ties), score cum + lp,
    lp = (logit - max) - log(sum exp(logit - max)); a finished row proposes itself extended by <pad> (lp 0, score cum); a row at
    cum = -inf proposes nothing;
  * per image the K best candidates by score (ties: lower parent slot, then lower rank) become slots 0..K-1; a chosen <eos> finishes
    the row, its length (tokens after <bos>) includes the <eos>;
  * the loop ends when every row is finished or after max_len - 1 steps; per image the slot with the highest cum / len^alpha wins
    (len = max_len - 1 for a row that never finished; ties: lower slot).

The self K/V caches are PHYSICALLY reordered by parent after every selection (index_select on the batch dimension) - deliberately a
different mechanism from the device's ancestor table."""
import math

import torch

from oracle import vitomr_oracle as O

NEG_INF = float("-inf")


def beam_generate(mem, lens_s, sd, num_heads, prec, K, max_len, alpha=1.0, bos_idx=0, pad_idx=1, eos_idx=2, prefix="decoder."):
    """mem: packed memory (sum(lens_s), E) (float64 for a float64 run).  Returns a dict:
    seqs / log_probs / mask  - the chosen hypotheses after mask_and_clip (as cached_beam_generate returns them),
    cum                      - (n,) float64 cumulative log-prob of the chosen hypotheses, best (n,) their slots,
    slot_seqs / slot_lps / slot_cum / slot_len / slot_fin - every slot as the loop ended (seqs (n*K, max_len) unclipped; len 0 = running),
    margins                  - per step, the smallest gap over the images between the K-th and (K+1)-th candidate score (inf if none),
    steps                    - steps run."""
    n = len(lens_s)
    R = n * K
    st = O.DecodeState(mem, lens_s, sd, num_heads, prec, prefix)
    # the memory repeated K times per image (K materialised copies of its cross K/V)
    st.k_cross = [[k for k in ks for _ in range(K)] for ks in st.k_cross]
    st.v_cross = [[v for v in vs for _ in range(K)] for vs in st.v_cross]
    st.B = R
    st.k_self = [torch.zeros(R, *c.shape[1:], dtype=c.dtype) for c in st.k_self]
    st.v_self = [torch.zeros(R, *c.shape[1:], dtype=c.dtype) for c in st.v_self]
    seqs = torch.full((R, max_len), pad_idx, dtype=torch.long)
    seqs[:, 0] = bos_idx
    lps = torch.zeros(R, max_len, dtype=torch.float64)
    cum = torch.full((R,), NEG_INF, dtype=torch.float64)
    cum[::K] = 0.0
    fin = torch.zeros(R, dtype=torch.bool)
    ln = torch.zeros(R, dtype=torch.long)
    margins = []
    steps = 0
    for t in range(1, max_len):
        logits = O.decode_step(st, seqs[:, t - 1], t).to(torch.float64)
        steps += 1
        parent = torch.arange(R)
        ntok = torch.full((R,), pad_idx, dtype=torch.long)
        nlp = torch.zeros(R, dtype=torch.float64)
        ncum = torch.full((R,), NEG_INF, dtype=torch.float64)
        nfin = torch.ones(R, dtype=torch.bool)
        nln = torch.zeros(R, dtype=torch.long)
        step_margin = math.inf
        for i in range(n):
            cands = []   # (score, parent slot, rank, token, lp)
            for k in range(K):
                r = i * K + k
                c = float(cum[r])
                if c == NEG_INF:
                    continue
                if bool(fin[r]):
                    cands.append((c, k, 0, pad_idx, 0.0))
                    continue
                lg = logits[r]
                m = lg.max()
                lse = torch.log(torch.exp(lg - m).sum())
                order = torch.sort(lg, descending=True, stable=True).indices[:K]   # ties: lower index first
                for rank, v in enumerate(order.tolist()):
                    lpv = float((lg[v] - m) - lse)
                    cands.append((c + lpv, k, rank, v, lpv))
            cands.sort(key=lambda x: (-x[0], x[1], x[2]))
            if len(cands) > K:
                step_margin = min(step_margin, cands[K - 1][0] - cands[K][0])
            for j, (sc, pk, _, tok, lpv) in enumerate(cands[:K]):
                row, pr = i * K + j, i * K + pk
                parent[row] = pr
                ntok[row] = tok
                nlp[row] = lpv
                ncum[row] = sc
                if bool(fin[pr]):
                    nln[row] = ln[pr]
                elif tok == eos_idx:
                    nln[row] = t
                else:
                    nfin[row] = False
            # (slots without a candidate stay dead: their own lineage + <pad>, cum -inf, finished)
        margins.append(step_margin)
        for l in range(st.L):
            st.k_self[l] = st.k_self[l].index_select(0, parent)
            st.v_self[l] = st.v_self[l].index_select(0, parent)
        seqs = seqs.index_select(0, parent)
        lps = lps.index_select(0, parent)
        seqs[:, t] = ntok
        lps[:, t] = O._r(nlp, prec)
        cum, fin, ln = ncum, nfin, nln
        if bool(fin.all()):
            break
    length = torch.where(fin, ln, torch.full_like(ln, max_len - 1)).to(torch.float64)
    score = torch.where(cum == NEG_INF, cum, cum / length.pow(alpha)).view(n, K)
    best = torch.argmax(score, dim=1)   # first maximum: lower slot on ties
    rows = torch.arange(n) * K + best
    s, lp, mask = O.mask_and_clip(seqs[rows], lps[rows], eos_idx, pad_idx)
    return dict(seqs=s, log_probs=lp, mask=mask, cum=cum[rows], best=best, slot_seqs=seqs, slot_lps=lps, slot_cum=cum,
                slot_len=torch.where(fin, ln, torch.zeros_like(ln)), slot_fin=fin, margins=margins, steps=steps)


def rescore(mem, lens_s, sd, num_heads, prec, seqs, eos_idx=2, prefix="decoder."):
    """Teacher-forced float64 re-scoring: sum over each row's tokens after <bos> (up to and including its first <eos>) of
    log_softmax(logits)[token], with the row decoded on its own memory."""
    n = len(lens_s)
    st = O.DecodeState(mem, lens_s, sd, num_heads, prec, prefix)
    tot = torch.zeros(n, dtype=torch.float64)
    done = torch.zeros(n, dtype=torch.bool)
    for t in range(1, seqs.shape[1]):
        logits = O.decode_step(st, seqs[:, t - 1], t).to(torch.float64)
        lp = torch.log_softmax(logits, dim=-1).gather(1, seqs[:, t:t + 1]).squeeze(1)
        tot += torch.where(done, torch.zeros_like(lp), lp)
        done |= seqs[:, t] == eos_idx
    return tot
