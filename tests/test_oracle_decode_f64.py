"""oracle.DecodeState / decode_step in float64: the self K/V caches take the memory's dtype, so a float64 run stays float64 end to end
and can serve as the high-precision reference of the decode kernels (tests/test_gpu_decode_forms.py).  CPU only."""
import torch
import torch.nn.functional as F

from oracle import vitomr_oracle as O


def _tiny_sd(E=8, H=2, Fd=16, V=6, T=8, L=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    sd = {"decoder.vocab_embedding.weight": r(V, E), "decoder.pos_embedding": r(T, E),
          "decoder.decoder_blocks.norm.weight": 1 + 0.1 * r(E), "decoder.decoder_blocks.norm.bias": 0.1 * r(E),
          "decoder.unembed.weight": r(V, E), "decoder.unembed.bias": r(V)}
    for l in range(L):
        p = f"decoder.decoder_blocks.layers.{l}."
        for a in ("self_attn", "multihead_attn"):
            sd[p + a + ".in_proj_weight"], sd[p + a + ".in_proj_bias"] = 0.4 * r(3 * E, E), 0.1 * r(3 * E)
            sd[p + a + ".out_proj.weight"], sd[p + a + ".out_proj.bias"] = 0.4 * r(E, E), 0.1 * r(E)
        sd[p + "linear1.weight"], sd[p + "linear1.bias"] = 0.4 * r(Fd, E), 0.1 * r(Fd)
        sd[p + "linear2.weight"], sd[p + "linear2.bias"] = 0.3 * r(E, Fd), 0.1 * r(E)
        for n in ("norm1", "norm2", "norm3"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = 1 + 0.1 * r(E), 0.1 * r(E)
    return sd


def _mha(q_in, kv_in, in_w, in_b, out_w, out_b, H):
    """Written out by hand: rows of q_in attend to every row of kv_in (no mask)."""
    E = q_in.shape[-1]
    dh = E // H
    q = (q_in @ in_w[:E].T + in_b[:E]).reshape(-1, H, dh).transpose(0, 1)
    k = (kv_in @ in_w[E:2 * E].T + in_b[E:2 * E]).reshape(-1, H, dh).transpose(0, 1)
    v = (kv_in @ in_w[2 * E:].T + in_b[2 * E:]).reshape(-1, H, dh).transpose(0, 1)
    p = torch.softmax(q @ k.transpose(1, 2) / dh ** 0.5, dim=-1)
    return (p @ v).transpose(0, 1).reshape(-1, E) @ out_w.T + out_b


def _hand_logits(sd, mem, tokens, H):
    """A post-LN decoder layer stack on one sequence, float64 throughout: the last position's logits after len(tokens) steps."""
    px = "decoder."
    x = sd[px + "vocab_embedding.weight"][tokens] + sd[px + "pos_embedding"][:len(tokens)]
    L = sum(1 for k in sd if k.endswith("norm1.weight"))
    E = x.shape[1]
    for l in range(L):
        p = f"{px}decoder_blocks.layers.{l}."
        ln = lambda z, n, eps=1e-5: F.layer_norm(z, (E,), sd[p + n + ".weight"], sd[p + n + ".bias"], eps)  # noqa: E731
        sa = torch.stack([_mha(x[i:i + 1], x[:i + 1], sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"],
                               sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], H)[0] for i in range(len(tokens))])
        x = ln(x + sa, "norm1")
        ca = _mha(x, mem, sd[p + "multihead_attn.in_proj_weight"], sd[p + "multihead_attn.in_proj_bias"],
                  sd[p + "multihead_attn.out_proj.weight"], sd[p + "multihead_attn.out_proj.bias"], H)
        x = ln(x + ca, "norm2")
        h = F.gelu(x @ sd[p + "linear1.weight"].T + sd[p + "linear1.bias"]) @ sd[p + "linear2.weight"].T + sd[p + "linear2.bias"]
        x = ln(x + h, "norm3")
    x = F.layer_norm(x, (E,), sd[px + "decoder_blocks.norm.weight"], sd[px + "decoder_blocks.norm.bias"], 1e-6)
    return (x @ sd[px + "unembed.weight"].T + sd[px + "unembed.bias"])[-1]


def test_decode_step_float64_end_to_end():
    H = 2
    sd = _tiny_sd()
    lens = [5, 3]
    mem = torch.randn(sum(lens), 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    st = O.DecodeState(mem, lens, sd, H, "fp32", t_cap=2)   # t_cap 2: the cache grows (and keeps its dtype) on the third step
    toks = torch.tensor([[0, 3, 5, 2], [0, 1, 1, 4]])
    for t in range(toks.shape[1]):
        logits = O.decode_step(st, toks[:, t], t)
        assert logits.dtype == torch.float64
        assert all(c.dtype == torch.float64 for c in st.k_self + st.v_self + [k for ks in st.k_cross for k in ks])
        for b, o in enumerate([0, lens[0]]):
            ref = _hand_logits(sd, mem[o:o + lens[b]], toks[b, :t + 1], H)
            assert float((logits[b] - ref).abs().max()) < 1e-12, (t, b)
    # the bf16 rounding points keep float64 as their container
    lb = O.decode_step(O.DecodeState(mem, lens, sd, H, "bf16"), toks[:, 0], 0)
    assert lb.dtype == torch.float64
    assert torch.equal(O.rbf16(torch.tensor([1.0 + 2 ** -9], dtype=torch.float64)), torch.tensor([1.0], dtype=torch.float64))


def test_decode_state_float32_unchanged():
    sd = {k: v.float() for k, v in _tiny_sd().items()}
    mem = torch.randn(7, 8, generator=torch.Generator().manual_seed(2))
    st = O.DecodeState(mem, [4, 3], sd, 2, "fp32")
    assert all(c.dtype == torch.float32 for c in st.k_self + st.v_self)
    assert O.decode_step(st, torch.tensor([0, 0]), 0).dtype == torch.float32
