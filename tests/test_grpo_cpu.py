"""GRPO update step, CPU side: the tensor-only reward helpers against the known answers of the reference's tests
(tests/test_omr_grpo_train.py:13-150, values restated) and the group-concatenated cross-attention layout of memory_group_size."""
import pytest
import torch

from conftest import VOCAB

from acai_omr_amd.train import grpo as G
from acai_omr_amd.train.autograd_path import group_cu


def _pad_idx():
    toks = [ln.strip() for ln in open(VOCAB) if ln.strip()]
    return toks.index("<pad>")


PAD = _pad_idx()


def test_calc_wellformedness_known_answers():
    assert torch.all(G.calc_wellformedness(torch.tensor([False, False, False]), torch.tensor([0, 0, 0])) == 1)
    s = G.calc_wellformedness(torch.tensor([False, False, False]), torch.tensor([2, 1, 0]))
    assert s[0] < s[1] and s[-1] == 1
    s = G.calc_wellformedness(torch.tensor([True, False, False]), torch.tensor([0, 2, 0]))
    assert s[0] == -3 and s[1] < 1
    s = G.calc_wellformedness(torch.tensor([True, False, True]), torch.tensor([20, 0, 0]))
    assert torch.equal(s, torch.tensor([-3.0, 1.0, -3.0]))


def test_calc_tedn_scores_zero_cost_is_one():
    assert torch.equal(G.calc_tedn_scores(torch.tensor([0.0, 0.0])), torch.tensor([1.0, 1.0]))
    assert float(G.calc_tedn_scores(torch.tensor([100.0]), alpha_t=0.01)) == pytest.approx(float(torch.exp(torch.tensor(-1.0))))


@pytest.mark.parametrize("rollouts, targets, prec, rec", [
    ([[0, 0, 0, 0], [0, 0, 0, 0]], [[0, 0, 0, 0], [0, 10, PAD, PAD]], [1, 1 / 4], [1, 1 / 2]),
    ([[20, 0, 0, 0], [0, 0, 0, 0]], [[0, 0, PAD], [0, 10, 0]], [1 / 4, 2 / 4], [1 / 2, 2 / 3]),
])
def test_calc_token_f1_known_answers(rollouts, targets, prec, rec):
    p, r = torch.tensor(prec), torch.tensor(rec)
    f1 = G.calc_token_f1(torch.tensor(rollouts), torch.tensor(targets), PAD)
    assert torch.equal(f1, 2 * p * r / (p + r + 1e-8))


@pytest.mark.parametrize("rollouts, n, expected", [
    ([[0, 0, 0, 0, 0, 5], [5, 6, 7, 8, 5, 5]], 2, [1 / 2, 0.0]),
    ([[0, 0, 0, 0, 0, 5], [5, 6, 7, 8, 5, 5]], 3, [0.0, 0.0]),
    ([[0, 0, 0, 0, PAD, PAD], [5, 5, 0, 5, 5, 5]], 2, [1.0, 0.0]),
    ([[0, 0, 0, 5, PAD, PAD], [5, 5, 0, 5, 5, 5]], 1, [2 / 3, 3 / 5]),
    ([[0, 0, 0, 0, PAD, PAD], [5, 5, 5, 5, 0, PAD]], 2, [1.0, 1.0]),
])
def test_calc_n_gram_penalty_known_answers(rollouts, n, expected):
    assert torch.equal(G.calc_n_gram_penalty(torch.tensor(rollouts), n, PAD), torch.tensor(expected))


def test_calc_repeat_penalty_orders_loops_first():
    ro = torch.tensor([[5, 0, 5, 5, 0, 0, PAD, PAD, PAD], [5, 6, 5, 6, 3, 7, 3, 4, 5]])
    p = G.calc_repeat_penalty(ro, PAD)
    assert p[0] > p[1]


def test_calc_len_penalty_known_answers():
    m = torch.full([2, 100], True)
    assert torch.equal(G.calc_len_penalty(m, torch.arange(100).unsqueeze(0).repeat(2, 1), PAD), torch.tensor([0.0, 0.0]))
    assert torch.equal(G.calc_len_penalty(m, torch.arange(105).unsqueeze(0).repeat(2, 1), PAD), torch.tensor([0.0, 0.0]))
    t = torch.arange(130).unsqueeze(0).repeat(2, 1)
    t[:, 105:] = PAD
    assert torch.equal(G.calc_len_penalty(m, t, PAD), torch.tensor([0.0, 0.0]))
    m = torch.full([2, 130], True)
    t = torch.arange(130).unsqueeze(0).repeat(2, 1)
    t[0, 105:] = PAD
    p = G.calc_len_penalty(m, t, PAD)
    assert p[0] > 0 and p[1] == 0
    p = G.calc_len_penalty(torch.full([2, 1], True), torch.arange(130).unsqueeze(0).repeat(2, 1), PAD)
    assert torch.equal(p, torch.tensor([1.0, 1.0]))


def test_expand_target_lmx_seqs_and_group_rewards():
    t = G.expand_target_lmx_seqs((torch.tensor([1, 2, 3]), torch.tensor([4])), 3, PAD, "cpu")
    assert t.shape == (6, 3)
    assert torch.equal(t[0], torch.tensor([1, 2, 3])) and torch.equal(t[2], torch.tensor([1, 2, 3]))
    assert torch.equal(t[3], torch.tensor([4, PAD, PAD])) and torch.equal(t[5], torch.tensor([4, PAD, PAD]))
    rc = G.RewardComponents(torch.ones(6), torch.zeros(6), torch.ones(6), torch.zeros(6), torch.full((6,), 0.5))
    r = G.calc_group_rewards(G.INITIAL_REWARD_CONFIG, rc, 2, 3)
    assert r.shape == (2, 3)
    assert torch.allclose(r, torch.full((2, 3), 7 + 2.5 - 2 * 0.5))


def test_initial_configs_are_the_reference_values():
    assert G.INITIAL_ROLLOUT_CONFIG == G.RolloutConfig(8, 768, 50, 1.1)
    assert G.INITIAL_LOSS_CONFIG == G.LossConfig(0.05, 0.1)
    assert G.INITIAL_UPDATE_CONFIG == G.UpdateConfig(0.2, 2, 1.0)
    cfg = G.GRPOConfig(G.INITIAL_ROLLOUT_CONFIG, G.INITIAL_REWARD_CONFIG, G.INITIAL_LOSS_CONFIG, G.INITIAL_UPDATE_CONFIG, 100, 100)
    assert cfg.get_configs()[3].epsilon == 0.2


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


@pytest.mark.parametrize("lens_t, lens_s, G_", [
    ([5, 1, 7, 2, 3, 1], [4, 9], 3),          # ragged rollouts, a rollout of length 1
    ([5, 1, 7], [4, 9, 2], 1),                # G = 1: the per-rollout layout itself
    ([1, 1, 1, 1, 1, 1, 1, 1], [6], 8),
    ([3, 4, 1, 6], [10, 2], 2),
])
def test_group_cu_concatenates_each_images_rollouts(lens_t, lens_s, G_):
    lens_q, lens_k = group_cu(lens_t, lens_s, G_)
    assert lens_k == lens_s
    # query sequence b = rows b*G .. b*G+G-1 of the packed stream: its bounds are every G-th entry of the rollouts' cu_seqlens
    assert _cu(lens_q) == _cu(lens_t)[::G_]
    assert len(lens_q) == len(lens_s)
    if G_ == 1:
        assert lens_q == lens_t


def test_group_cu_rejects_a_wrong_group_size():
    with pytest.raises(ValueError):
        group_cu([1, 2, 3], [4, 5], 2)
