"""The host mirror of the kernels' dropout masks (oracle/dropout_mirror.py) and the oracle's train-mode dropout hook.  CPU only.

The known-answer vectors are common.h's drop_hash compiled as plain C (gcc, 32-bit unsigned arithmetic); the thresholds are the C ABI's
(uint32_t)((double)p_f32 * 2^32) of the fp32 p the entry points receive."""
import pytest
import torch

from conftest import load_golden
from oracle import dropout_mirror as DM
from oracle import vitomr_oracle as O


@pytest.mark.parametrize("seed,row,col,h", [
    (0, 0, 0, 0x00000000),
    (777, 3, 5, 0x23DAFAD0),
    (123, 511, 383, 0xC4DF6F10),
    (0xFFFFFFFF, 70000, 4095, 0x3DECDF61),
    (42, 73745, 4095, 0x34A21487),
    (2147483600, 123456, 77, 0x1ECBD638),
])
def test_hash_known_answers(seed, row, col, h):
    assert int(DM.drop_hash(seed, row, col)) == h
    # vectorised: the same element inside a broadcast block
    blk = DM.drop_hash(seed, torch.tensor([[row], [row + 1]]), torch.tensor([[col - 1, col]]) if col else torch.tensor([[col, col + 1]]))
    assert int(blk[0, 1 if col else 0]) == h


@pytest.mark.parametrize("p,thr,thr_double", [(0.05, 214748368, 214748364), (0.1, 429496736, 429496729), (0.3, 1288490240, 1288490188),
                                              (0.5, 2147483648, 2147483648)])
def test_threshold_from_the_fp32_probability(p, thr, thr_double):
    assert DM.drop_threshold(p) == thr
    assert int(p * 4294967296.0) == thr_double      # what the double p would give: not the kernels' threshold (except at p = 0.5)
    assert DM.drop_scale(0.1) == float(torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(0.1, dtype=torch.float32)))


def test_keep_is_hash_at_or_above_the_threshold():
    """keep iff hash >= thr, exactly at the boundary; helpers agree with the raw hash in both coordinate systems."""
    h = DM.drop_hash(9, torch.arange(300).unsqueeze(1), torch.arange(200).unsqueeze(0))
    p = 0.3
    assert torch.equal(DM.dropout_keep(9, 300, 200, p), h >= DM.drop_threshold(p))
    rows = torch.tensor([5, 17, 299])
    assert torch.equal(DM.dropout_keep(9, rows, 200, p), (h >= DM.drop_threshold(p))[rows])
    # attention block (h = 1, queries of a sequence starting at packed row 40 of 120)
    assert torch.equal(DM.attn_keep(9, p, 1, 120, 40, 30, 200), (h >= DM.drop_threshold(p))[160:190])


def test_mask_statistics_at_p_0_1():
    """~10^6 elements at p = 0.1: keep rate overall and per row / column within binomial bounds (6 sigma), no correlation between
    neighbouring columns or rows, none between the masks of two heads over the same queries."""
    p, n = 0.1, 1024
    k = DM.attn_keep(2 ** 31 - 5, p, 0, n, 0, n, n).double()
    k1 = DM.attn_keep(2 ** 31 - 5, p, 1, n, 0, n, n).double()
    q = 1 - p
    assert abs(float(k.mean()) - q) < 6 * (q * p / k.numel()) ** 0.5
    sd_line = (n * q * p) ** 0.5
    assert float((k.sum(1) - n * q).abs().max()) < 6 * sd_line
    assert float((k.sum(0) - n * q).abs().max()) < 6 * sd_line

    def corr(a, b):
        a, b = a.flatten() - a.mean(), b.flatten() - b.mean()
        return float((a @ b) / (a.norm() * b.norm()))

    bar = 6 / (n * (n - 1)) ** 0.5
    assert abs(corr(k[:, :-1], k[:, 1:])) < bar
    assert abs(corr(k[:-1], k[1:])) < bar
    assert abs(corr(k, k1)) < bar
    d = DM.dropout_keep(77, n, n, p).double()
    assert abs(corr(d[:, :-1], d[:, 1:])) < bar and abs(float(d.mean()) - q) < 6 * (q * p / d.numel()) ** 0.5


def _tf_case():
    fx = load_golden("tf_small")
    cfg = fx["cfg"]
    return fx, cfg, list(zip(fx["imgs"], fx["lmx"]))


def test_oracle_dropout_hook_sites_and_identity():
    """drop=None is the eval oracle; a hook that answers None everywhere, or multiplies by exactly 1, changes nothing (bit for bit); the sites
    come in torch's order per layer (encoder: probabilities, dropout1, dropout, dropout2; head: 2; decoder: probabilities, dropout1, cross
    probabilities, dropout2, dropout, dropout3) with the geometry the GPU test maps onto the HIP packing."""
    fx, cfg, batch = _tf_case()
    sd = fx["state_dict"]
    ref, _ = O.teacher_forced_forward(batch, sd, cfg["enc_heads"], cfg["dec_heads"], cfg["P"], "fp32")
    seen = []

    def none_hook(site, kind, **g):
        seen.append((site, kind, g))
        return None

    def ones_hook(site, kind, **g):
        if kind == "add":
            return torch.ones(sum(g["lens"]), g["cols"])
        return lambda i, h: torch.ones(g["lens_q"][i], g["lens_k"][i])

    assert torch.equal(O.teacher_forced_forward(batch, sd, cfg["enc_heads"], cfg["dec_heads"], cfg["P"], "fp32", drop=none_hook)[0], ref)
    assert torch.equal(O.teacher_forced_forward(batch, sd, cfg["enc_heads"], cfg["dec_heads"], cfg["P"], "fp32", drop=ones_hook)[0], ref)
    names = [s for s, _, _ in seen]
    n_enc = cfg["enc_layers"]
    n_dec = sum(1 for k in sd if k.startswith("decoder.decoder_blocks.layers.") and k.endswith(".norm1.weight"))
    assert len(names) == 4 * n_enc + 1 + 6 * n_dec
    ft0 = cfg["enc_layers"] - cfg["ft_depth"]
    first = "encoder.fine_tune_blocks.layers.0." if ft0 == 0 else "encoder.frozen_blocks.layers.0."
    assert names[:4] == [first + s for s in ("self_attn", "dropout1", "dropout", "dropout2")]
    assert names[4 * n_enc] == "transition_head.2"
    d0 = "decoder.decoder_blocks.layers.0."
    assert names[4 * n_enc + 1:4 * n_enc + 7] == [d0 + s for s in ("self_attn", "dropout1", "multihead_attn", "dropout2", "dropout", "dropout3")]
    kinds = {s: k for s, k, _ in seen}
    assert kinds[d0 + "multihead_attn"] == "attn" and kinds[d0 + "dropout3"] == "add"
    g = dict((s, g) for s, _, g in seen)
    T = len(max(fx["lmx"], key=len)) - 1
    assert g[d0 + "self_attn"]["lens_q"] == [T] * len(batch) and g[d0 + "multihead_attn"]["lens_k"] == g["transition_head.2"]["lens"]


def test_oracle_residual_dropout_sites_are_torchs():
    """The oracle's residual dropout sites against torch's own layers in float64: nn.TransformerEncoderLayer / nn.TransformerDecoderLayer
    (post-LN, GELU) in train mode, their nn.Dropout modules' outputs replaced by forward hooks with the mirror's masks, the attention
    probabilities left undropped on both sides.  Same output: every residual site is where torch applies it, with the same mask."""
    torch.manual_seed(0)
    E, H, F_, p = 32, 2, 48, 0.3
    enc = torch.nn.TransformerEncoderLayer(E, H, F_, dropout=p, activation="gelu", batch_first=True).double().train()
    dec = torch.nn.TransformerDecoderLayer(E, H, F_, dropout=p, activation="gelu", batch_first=True).double().train()
    for layer in (enc, dec):
        for m in (layer.self_attn, getattr(layer, "multihead_attn", None)):
            if m is not None:
                m.dropout = 0.0
    L, S = 9, 13
    x = torch.randn(1, L, E, dtype=torch.float64)
    mem = torch.randn(1, S, E, dtype=torch.float64)
    seeds = {}

    def mult(site, rows, cols):
        s = seeds.setdefault(site, 1000 + len(seeds))
        return DM.multiplier(DM.dropout_keep(s, rows, cols, p), p)

    def install(prefix, layer):
        hs = []
        for name, mod in layer.named_modules():
            if isinstance(mod, torch.nn.Dropout):
                site = prefix + name
                hs.append(mod.register_forward_hook(lambda m, i, o, site=site: i[0] * mult(site, i[0].shape[-2], i[0].shape[-1]).view(i[0].shape)))
        return hs

    def oracle_drop(site, kind, **g):
        return None if kind == "attn" else mult(site, sum(g["lens"]), g["cols"])

    sd = {"e." + k: v for k, v in enc.state_dict().items()}
    sd.update({"d." + k: v for k, v in dec.state_dict().items()})
    hs = install("e.", enc) + install("d.", dec)
    try:
        with torch.no_grad():
            y_enc = enc(x)
            y_dec = dec(x, mem, tgt_mask=torch.nn.Transformer.generate_square_subsequent_mask(L, dtype=torch.float64),
                        tgt_is_causal=True)
    finally:
        for h in hs:
            h.remove()
    assert set(seeds) == {"e.dropout1", "e.dropout", "e.dropout2", "d.dropout1", "d.dropout2", "d.dropout", "d.dropout3"}
    o_enc = O.encoder_layer(x[0], [L], sd, "e.", H, "fp32", drop=oracle_drop)
    o_dec = O.decoder_layer_tf(x[0], mem[0], [L], [S], sd, "d.", H, "fp32", None, drop=oracle_drop)
    assert float((o_enc - y_enc[0]).abs().max()) < 1e-12
    assert float((o_dec - y_dec[0]).abs().max()) < 1e-12
    # and the masks matter: without them the outputs differ
    assert float((O.encoder_layer(x[0], [L], sd, "e.", H, "fp32") - y_enc[0]).abs().max()) > 1e-3
