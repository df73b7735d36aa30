"""The GRPO policy-update step (acai_omr/train/omr_grpo_train.py:120-376, the configs of acai_omr/utils/utils.py:17-105): objective, entropy
bonus, teacher-forced policy forward / backward and the optimizer step that consume rollouts and their rewards.

Same names and argument orders as the reference, so code written for omr_grpo_train.py ports.  What differs:
  * the objective and the entropy bonus come from ONE fused HIP pass over the theta logits (acai_grpo_objective_fwd / _bwd); there is no CPU
    path, as elsewhere in the package.  An entropy term with p_c == 0 counts 0 where the reference gives NaN (only -inf logits produce it);
  * the policy forward runs on the UNEXPANDED image memory (OMRDecoder.forward(memory_group_size=G)): the reference's
    expand_img_latent_for_rollout copies it G times, and every layer projects each copy;
  * rewards: grpo_update takes a `reward_fn` that returns the (B, G) raw rewards.  The tensor-only reward helpers are here, and so is a
    reward that runs from the package alone: the TOKEN-level edit cost (calc_token_edit_costs: Levenshtein distance over LMX tokens, one HIP
    launch on the rollouts where they lie, acai_edit_distance) stands in for the reference's tree edit cost in token_reward_rollouts /
    make_token_reward_fn.  Not ported: calc_edit_costs itself (TEDn on MusicXML trees through olimpic_app) and the delinearizer's
    well-formedness counts.  With a token automaton (grammar.TokenAutomaton, `grammar=`) the well-formedness term is computed from the
    automaton instead - violations and "ended with an allowed <eos>" from one scan launch over the rollouts (acai_grammar_scan) - and the
    rollouts themselves can be constrained by it (grpo_update(grammar=), validation_loop(grammar=));
  * rollouts may go through continuously refilled decode rows instead of one static batch (grpo_update(rollout_slots=...), and always in
    validation_loop): the same draws per rollout, no B * G <= max batch size limit, and a rollout that never draws <eos> does not hold the
    finished ones' rows to max_actions;
  * grpo_update(fused_clip=True) clips inside the fused AdamW step (optim.FusedAdamW.step(max_grad_norm=1.0)) instead of through
    torch.nn.utils.clip_grad_norm_; off by default, the reference's call stays."""
from dataclasses import dataclass

import torch

from .. import ops
from ..optim import FusedAdamW
from . import autograd_path as AP


# ---- configs (utils.py:17-105) ----------------------------------------------------------------------------------------------------------
@dataclass
class RolloutConfig:
    group_size: int
    max_actions: int
    top_k: int
    temperature: float


@dataclass
class RewardComponents:
    tedn_scores: torch.Tensor | float
    wellformedness_scores: torch.Tensor | float
    f1_scores: torch.Tensor | float
    repeat_penalty: torch.Tensor | float
    len_penalty: torch.Tensor | float

    def __add__(self, other):
        return RewardComponents(*(a + b for a, b in zip(self._vals(), other._vals())))

    def __truediv__(self, divisor):
        return RewardComponents(*(a / divisor for a in self._vals()))

    def _vals(self):
        return (self.tedn_scores, self.wellformedness_scores, self.f1_scores, self.repeat_penalty, self.len_penalty)

    def avg_over_rollouts(self):
        return RewardComponents(*(a.mean().item() for a in self._vals()))

    def to_dict(self):
        return {"tedn_scores": self.tedn_scores, "wellformedness_scores": self.wellformedness_scores, "f1_scores": self.f1_scores,
                "repeat_penalty": self.repeat_penalty, "len_penalty": self.len_penalty}


@dataclass
class RewardConfig:
    lambda_tedn: float
    lambda_well_formed: float
    lambda_f1: float
    lambda_repeat: float
    lambda_len: float
    alpha_tedn: float
    alpha_well_formed: float
    gamma: float
    delta: int
    tau: int


@dataclass
class LossConfig:
    entropy_beta: float
    lambda_ce: float


@dataclass
class UpdateConfig:
    epsilon: float
    update_epochs: int
    max_grad_norm: float


@dataclass
class GRPOConfig:
    rollout_config: RolloutConfig
    reward_config: RewardConfig
    loss_config: LossConfig
    update_config: UpdateConfig
    mini_validation_freq: int
    checkpoint_freq: int

    def get_configs(self):
        return self.rollout_config, self.reward_config, self.loss_config, self.update_config


class StepCounter:
    def __init__(self):
        self.global_step = 0


# the reference's initial values (omr_grpo_train.py:30-72)
LR = 1e-6
ADAMW_BETAS = (0.9, 0.95)
ADAMW_WEIGHT_DECAY = 0.0
TRAIN_BATCH_SIZE = 16
INITIAL_ROLLOUT_CONFIG = RolloutConfig(group_size=8, max_actions=768, top_k=50, temperature=1.1)
INITIAL_REWARD_CONFIG = RewardConfig(lambda_tedn=7, lambda_well_formed=1.5, lambda_f1=2.5, lambda_repeat=2, lambda_len=2, alpha_tedn=0.01,
                                     alpha_well_formed=0.25, gamma=3, delta=5, tau=50)
INITIAL_LOSS_CONFIG = LossConfig(entropy_beta=0.05, lambda_ce=0.1)
INITIAL_UPDATE_CONFIG = UpdateConfig(epsilon=0.2, update_epochs=2, max_grad_norm=1.0)


# ---- rewards (tensor-only helpers, omr_grpo_train.py:121-226) ------------------------------------------------------------------------------
def expand_target_lmx_seqs(target_lmx_seqs, group_size, pad_idx, device):
    """(B) ragged targets -> (B*G, Lmax) padded with pad_idx, each target repeated for its group's rollouts."""
    L = max(int(t.shape[0]) for t in target_lmx_seqs)
    out = torch.full((len(target_lmx_seqs), L), pad_idx, dtype=target_lmx_seqs[0].dtype, device=device)
    for i, t in enumerate(target_lmx_seqs):
        out[i, :t.shape[0]] = t.to(device)
    return out.unsqueeze(1).expand(-1, group_size, -1).flatten(start_dim=0, end_dim=1)


def calc_tedn_scores(edit_costs, alpha_t=0.01):
    return torch.exp(-alpha_t * edit_costs)


def calc_wellformedness(catastrophic_errors, minor_errors, gamma=3.0, alpha_w=0.2):
    return torch.exp(-alpha_w * minor_errors).masked_fill(catastrophic_errors, -gamma)


def calc_token_f1(rollouts, target_lmx_seqs, pad_idx):
    num_predictions = (rollouts != pad_idx).sum(dim=-1)
    num_targets = (target_lmx_seqs != pad_idx).sum(dim=-1)
    n = min(rollouts.shape[-1], target_lmx_seqs.shape[-1])
    preds, targets = rollouts[:, :n], target_lmx_seqs[:, :n]
    true_positives = ((preds == targets) & (targets != pad_idx)).sum(dim=-1)
    precision = true_positives / (num_predictions + 1e-8)
    recall = true_positives / (num_targets + 1e-8)
    return 2 * precision * recall / (precision + recall + 1e-8)


def calc_n_gram_penalty(rollouts, n, pad_idx):
    """Share of non-overlapping n-grams equal to the one before them (n-grams holding <pad> left out)."""
    n_grams = rollouts.unfold(dimension=-1, size=n, step=n)
    prev_n_grams, next_n_grams = n_grams[:, :-1, :], n_grams[:, 1:, :]
    pad_mask = torch.any(next_n_grams == pad_idx, dim=-1)
    repeats = torch.all(prev_n_grams == next_n_grams, dim=-1) & ~pad_mask
    return repeats.sum(dim=-1) / ((~pad_mask).sum(dim=-1) + 1e-8)


def calc_repeat_penalty(rollouts, pad_idx, n_values=(1, 2, 3, 4)):
    total = 0
    for n in n_values:
        total += calc_n_gram_penalty(rollouts, n, pad_idx)
    return total / len(n_values)


def calc_len_penalty(rollout_mask, target_lmx_seqs, pad_idx, delta=10, tau=100):
    len_diffs = torch.abs(rollout_mask.sum(dim=-1) - (target_lmx_seqs != pad_idx).sum(dim=-1))
    len_diffs = len_diffs.masked_fill(len_diffs < delta, 0)
    penalty = torch.exp((torch.log(torch.tensor(2)) / tau) * len_diffs) - 1
    return torch.clip(penalty, max=1.0)


def calc_group_rewards(reward_config: RewardConfig, reward_components: RewardComponents, num_groups, group_size):
    c, rc = reward_components, reward_config
    rewards = (rc.lambda_tedn * c.tedn_scores + rc.lambda_well_formed * c.wellformedness_scores + rc.lambda_f1 * c.f1_scores
               - rc.lambda_repeat * c.repeat_penalty - rc.lambda_len * c.len_penalty)
    return rewards.view(num_groups, group_size)


# ---- a reward without the external tree-edit tool: token-level edit costs on the device ------------------------------------------------------
def calc_token_edit_costs(rollouts, rollout_mask, target_lmx_seqs, pad_idx, group_size=1):
    """Levenshtein distance over LMX tokens of each rollout (its rollout_mask positions, <bos> / <eos> included as they stand) to its target
    (the non-pad entries, counted as calc_len_penalty counts them: targets are padded on the right), as float (R,).  target_lmx_seqs is either
    the expanded (R, L) tensor grpo_update hands to reward_fn (group_size=1) or the unexpanded (B, L) one with group_size=G."""
    target_lens = (target_lmx_seqs != pad_idx).sum(dim=-1, dtype=torch.int32)
    return ops.edit_distance(rollouts, rollout_mask, target_lmx_seqs, target_lens, group=group_size).float()


def calc_grammar_wellformedness(rollouts, rollout_mask, grammar, gamma=3.0, alpha_w=0.2):
    """calc_wellformedness from a token automaton: minor errors = the rollout's transitions the automaton forbids, catastrophic = the rollout
    did not end with an allowed <eos> (ops.grammar_scan: one launch on the rollouts where they lie).  This stands in for the delinearizer's
    verdict as the token edit cost stands in for TEDn: it says what the automaton knows - for one learned from a corpus, whether the rollout's
    n-grams occur in that corpus - not whether the LMX delinearizes."""
    violations, complete = ops.grammar_scan(rollouts, rollout_mask, grammar)
    return calc_wellformedness(~complete, violations.float(), gamma=gamma, alpha_w=alpha_w)


def token_reward_rollouts(reward_config: RewardConfig, rollouts, rollout_mask, target_lmx_seqs, num_groups, group_size, pad_idx, grammar=None):
    """reward_rollouts (omr_grpo_train.py:227-237) with the token-level edit cost in the place of the tree edit cost:
    tedn_scores = calc_tedn_scores(calc_token_edit_costs(...), alpha_tedn).  Without a grammar wellformedness_scores is a zeros tensor: the
    catastrophic / minor error counts come from delinearizing the LMX string, and the delinearizer is not part of this package.  With
    grammar (a grammar.TokenAutomaton) it is calc_grammar_wellformedness(rollouts, rollout_mask, grammar, gamma, alpha_well_formed): the
    automaton's verdict in the delinearizer's place.  The other three components are the reference's.  target_lmx_seqs: the expanded
    (B*G, L) targets.  Returns (raw_group_rewards (B, G), RewardComponents)."""
    token_edit_costs = calc_token_edit_costs(rollouts, rollout_mask, target_lmx_seqs, pad_idx)
    tedn_scores = calc_tedn_scores(token_edit_costs, alpha_t=reward_config.alpha_tedn)
    if grammar is None:
        wellformedness_scores = torch.zeros_like(tedn_scores)
    else:
        wellformedness_scores = calc_grammar_wellformedness(rollouts, rollout_mask, grammar, gamma=reward_config.gamma,
                                                            alpha_w=reward_config.alpha_well_formed).to(tedn_scores.device)
    f1_scores = calc_token_f1(rollouts, target_lmx_seqs, pad_idx)
    repeat_penalty = calc_repeat_penalty(rollouts, pad_idx)
    len_penalty = calc_len_penalty(rollout_mask, target_lmx_seqs, pad_idx, delta=reward_config.delta, tau=reward_config.tau)
    reward_components = RewardComponents(tedn_scores, wellformedness_scores, f1_scores, repeat_penalty, len_penalty)
    raw_group_rewards = calc_group_rewards(reward_config, reward_components, num_groups, group_size)
    return raw_group_rewards, reward_components


def make_token_reward_fn(reward_config: RewardConfig, pad_idx, grammar=None):
    """A `reward_fn` for grpo_update built from token_reward_rollouts: the group shape is read off the batch and the expanded targets.
    grammar: the token automaton of the well-formedness term (token_reward_rollouts); None leaves that term at zero."""
    def reward_fn(rollouts, rollout_mask, target_lmx_seqs, batch):
        num_groups = len(batch)
        return token_reward_rollouts(reward_config, rollouts, rollout_mask, target_lmx_seqs, num_groups, rollouts.shape[0] // num_groups, pad_idx,
                                     grammar=grammar)
    return reward_fn


# ---- objective and entropy (omr_grpo_train.py:240-283) through the fused op -------------------------------------------------------------
def calc_grpo_objective_and_entropy_bonus(theta_logits, rollouts, rollout_attention_mask, old_policy_log_probs, advantages, epsilon, num_groups):
    """(calc_grpo_objective(...), calc_entropy_bonus(theta_logits, rollout_attention_mask, V)) from one kernel pass over the logits."""
    return AP.GrpoObjectiveFn.apply(theta_logits, rollouts, rollout_attention_mask, old_policy_log_probs, advantages, float(epsilon), int(num_groups))


def calc_grpo_objective(theta_logits, rollouts, rollout_attention_mask, old_policy_log_probs, advantages, epsilon, num_groups):
    return calc_grpo_objective_and_entropy_bonus(theta_logits, rollouts, rollout_attention_mask, old_policy_log_probs, advantages, epsilon,
                                                 num_groups)[0]


def calc_policy_theta_entropy(theta_logits, rollout_attention_mask):
    """Per-rollout mean entropy (R,), the fused op's per-rollout statistic, without a gradient (calc_entropy_bonus is the differentiable form)."""
    R, T, V = theta_logits.shape
    dev = theta_logits.device
    lg = theta_logits.detach().contiguous()
    if lg.data_ptr() % 16:
        lg = lg.clone()
    # (zero actions / advantages: the entropy half of the pass does not read them)
    _, _, rowstat = ops.grpo_objective_fwd(lg, torch.zeros(R, T + 1, dtype=torch.int64, device=dev), rollout_attention_mask.contiguous(),
                                           torch.zeros(R, T + 1, device=dev), torch.zeros(R, device=dev), 0.8, 1.2, 1, float(torch.log(torch.tensor(V))))
    return rowstat[:, 1].clone()


def calc_entropy_bonus(theta_logits, rollout_attention_mask, vocab_size):
    R, T, V = theta_logits.shape
    assert V == vocab_size, "calc_entropy_bonus: vocab_size must be the logits' last dimension"
    dev = theta_logits.device
    rollouts = torch.zeros(R, T + 1, dtype=torch.int64, device=dev)
    return calc_grpo_objective_and_entropy_bonus(theta_logits, rollouts, rollout_attention_mask, torch.zeros(R, T + 1, device=dev),
                                                 torch.zeros(R, device=dev), 0.2, 1)[1]


def calc_teacher_forced_ce_loss(policy_theta, unexpanded_img_latent, unexpanded_latent_attention_mask, unexpanded_target_lmx_seqs, ce_loss_fn):
    logits, target_seqs = policy_theta.forward_teacher_forced(unexpanded_img_latent, unexpanded_latent_attention_mask, unexpanded_target_lmx_seqs,
                                                              checkpoint_grads=True)
    return ce_loss_fn(logits, target_seqs)


# ---- the update step (omr_grpo_train.py:308-376) ---------------------------------------------------------------------------------------
def _rollouts_grouped(old_policy, img_latent, latent_attention_mask, group_size, rollout_config, uniforms, grammar=None):
    """cached_forward_rollout_policy(expand_img_latent_for_rollout(...), group_size=G) without making the G copies: the cached decode reads
    one memory per image already (group_size), so the per-image latent goes in as it is."""
    from .. import engine as EG
    blocks = old_policy.decoder.decoder_blocks
    mem32, lens = EG.unpad_rows(img_latent, latent_attention_mask)
    blocks.prepare_caches_packed(mem32, None, lens, group_size=group_size)
    eng = blocks.engine(old_policy.decoder.pos_embedding.device)
    seqs, lps, _ = eng.sample(rollout_config.max_actions, rollout_config.top_k, rollout_config.temperature, uniforms=uniforms, grammar=grammar)
    return old_policy.mask_and_clip_seqs(seqs.clone(), lps.clone())


def _rollouts_continuous(old_policy, img_latent, latent_attention_mask, group_size, rollout_config, uniforms, slots, grammar=None):
    """The same rollouts through `slots` continuously refilled decode rows (GRPOViTOMR.cached_continuous_rollout_policy): B * G may exceed
    the cache's max batch size, at the price of one cross K/V projection per rollout instead of one per image."""
    if grammar is not None:
        return old_policy.cached_constrained_continuous_rollout_policy(img_latent, latent_attention_mask, grammar, rollout_config.max_actions,
                                                                       rollout_config.top_k, rollout_config.temperature, slots=slots,
                                                                       group_size=group_size, uniforms=uniforms)
    return old_policy.cached_continuous_rollout_policy(img_latent, latent_attention_mask, rollout_config.max_actions, rollout_config.top_k,
                                                       rollout_config.temperature, slots=slots, group_size=group_size, uniforms=uniforms)


def loop_rate(rollouts, rollout_mask, loop_guard):
    """The share of rollouts a loops.LoopGuard's rule flags (loops.scan_repeats: one launch over the rollouts where they lie), as a 0-dim
    fp32 tensor on their device - no host sync.  A diagnostic only: rewards do not see it."""
    from ..loops import scan_repeats
    return scan_repeats(rollouts, loop_guard, lens=rollout_mask).looped.float().mean()


def grpo_update(old_policy, policy_theta, optimizer, batch, grpo_config: GRPOConfig, ce_loss_fn, device, logger=None, counter=None, *, reward_fn,
                uniforms=None, rollout_slots=None, loop_guard=None, grammar=None, fused_clip=False):
    """One GRPO minibatch update.  batch: list of (image, target_lmx_seq, target_musicxml_str).  reward_fn(rollouts, rollout_mask, target_lmx_seqs,
    batch) -> (B, G) raw rewards, or (rewards, RewardComponents).  uniforms (R, max_actions): the rollout draws (cached_forward_rollout_policy).
    rollout_slots: None = one static batch of B * G rollout rows (B * G <= the cache's max batch size); an integer = that many decode rows
    refilled as rollouts finish, for any B * G.  grammar: a grammar.TokenAutomaton that constrains the rollouts
    (cached_forward_rollout_policy(grammar=)): old_policy_log_probs are then the constrained policy's, while the theta logits of the ratio
    stay unconstrained - pass the same automaton to make_token_reward_fn to reward what it checks.  fused_clip: clip inside the optimizer's
    own launches (`optimizer.step(max_grad_norm=1.0)`, optimizer an `optim.FusedAdamW`) instead of `torch.nn.utils.clip_grad_norm_`: one read of
    the gradients instead of three, a non-finite norm skips the step, and `optimizer.grad_norm` / `clip_coef` / `skipped_steps` report it without
    a host round trip.  loop_guard: a loops.LoopGuard - with a logger, the share of this minibatch's rollouts its rule flags is logged
    (`logger.log_loop_rate(rate, step)`, loop_rate above); the rollouts are NOT guarded and the rewards are untouched.  Returns (avg loss
    over update epochs, avg CE loss, avg raw reward, avg reward components or None)."""
    from ..loops import check_guard
    check_guard(loop_guard)
    if fused_clip and not isinstance(optimizer, FusedAdamW):
        raise ValueError(f"grpo_update: fused_clip needs an optim.FusedAdamW, got {type(optimizer).__name__}")
    rollout_config, reward_config, loss_config, update_config = grpo_config.get_configs()
    dev_type = torch.device(device).type
    pad_idx = old_policy.decoder.pad_idx
    unexpanded_imgs, unexpanded_target_lmx_seqs, _ = zip(*batch)
    unexpanded_imgs = [img.to(device, non_blocking=True) for img in unexpanded_imgs]
    unexpanded_target_lmx_seqs = [t.to(device, non_blocking=True) for t in unexpanded_target_lmx_seqs]
    group_size = rollout_config.group_size
    num_groups = len(batch)

    with torch.no_grad(), torch.autocast(device_type=dev_type, dtype=torch.bfloat16):
        unexpanded_img_latent, unexpanded_latent_attention_mask = old_policy.encoder(unexpanded_imgs)
        unexpanded_img_latent = old_policy.transition_head(unexpanded_img_latent)
        if rollout_slots is None:
            rollouts, old_policy_log_probs, rollout_mask = _rollouts_grouped(old_policy, unexpanded_img_latent, unexpanded_latent_attention_mask,
                                                                             group_size, rollout_config, uniforms, grammar)
        else:
            rollouts, old_policy_log_probs, rollout_mask = _rollouts_continuous(old_policy, unexpanded_img_latent, unexpanded_latent_attention_mask,
                                                                                group_size, rollout_config, uniforms, int(rollout_slots), grammar)

    target_lmx_seqs = expand_target_lmx_seqs(unexpanded_target_lmx_seqs, group_size, pad_idx, device)
    got = reward_fn(rollouts, rollout_mask, target_lmx_seqs, batch)
    raw_group_rewards, reward_components = got if isinstance(got, tuple) else (got, None)
    raw_group_rewards = raw_group_rewards.to(device).float().view(num_groups, group_size)
    if logger is not None:
        logger.log_raw_reward_stats(raw_group_rewards, counter.global_step)
        if reward_components is not None:
            logger.log_raw_reward_components(reward_components, counter.global_step)
        if loop_guard is not None:
            logger.log_loop_rate(loop_rate(rollouts, rollout_mask, loop_guard), counter.global_step)
    group_advantages = (raw_group_rewards - raw_group_rewards.mean(dim=-1, keepdim=True)) / (raw_group_rewards.std(dim=-1, keepdim=True) + 1e-8)
    advantages = group_advantages.view(-1)
    if logger is not None:
        logger.log_group_advantages(group_advantages, counter.global_step)
    right_shifted_rollouts, rollout_attention_mask = old_policy.prepare_rollouts_for_policy_theta(rollouts, rollout_mask)
    unexpanded_img_latent = unexpanded_img_latent.float()   # (the decoder's fp32 memory stream; B*S rows, not B*G*S)

    batch_overall_loss = 0.0
    batch_ce_loss = 0.0
    update_epochs = update_config.update_epochs
    with torch.autocast(device_type=dev_type, dtype=torch.bfloat16):
        for _ in range(update_epochs):
            # both decoder passes of the epoch read the same per-image memory: each layer projects it once (shared_cross_kv)
            with AP.shared_cross_kv():
                theta_logits = policy_theta.decoder(right_shifted_rollouts, unexpanded_img_latent, rollout_attention_mask, unexpanded_latent_attention_mask,
                                                    checkpoint_grads=True, memory_group_size=group_size)
                grpo_objective, entropy_bonus = calc_grpo_objective_and_entropy_bonus(theta_logits, rollouts, rollout_attention_mask,
                                                                                      old_policy_log_probs, advantages, update_config.epsilon, num_groups)
                if loss_config.lambda_ce:
                    ce_loss = calc_teacher_forced_ce_loss(policy_theta, unexpanded_img_latent, unexpanded_latent_attention_mask,
                                                          unexpanded_target_lmx_seqs, ce_loss_fn)
                else:
                    # quirk kept: no CE term at lambda_ce == 0 (the reference's `ce_loss = 0` then crashes on `.item()`; here it counts 0)
                    ce_loss = torch.zeros((), device=theta_logits.device)
            if logger is not None:
                logger.log_raw_objective_components(grpo_objective, entropy_bonus, ce_loss, counter.global_step)
            loss = -(grpo_objective + loss_config.entropy_beta * entropy_bonus - loss_config.lambda_ce * ce_loss)
            batch_overall_loss += loss.item()   # (the reference's two syncs per epoch, nothing more)
            batch_ce_loss += ce_loss.item()
            if logger is not None:
                logger.log_overall_loss(loss, counter.global_step)
            loss.backward()
            # quirk kept: max_norm is the literal 1.0 of omr_grpo_train.py:367 - UpdateConfig.max_grad_norm is not read
            if fused_clip:
                optimizer.step(max_grad_norm=1.0)
            else:
                torch.nn.utils.clip_grad_norm_(policy_theta.parameters(), max_norm=1.0)
                optimizer.step()
            optimizer.zero_grad()
            if counter is not None:
                counter.global_step += 1

    avg_components = reward_components.avg_over_rollouts() if reward_components is not None else None
    return batch_overall_loss / update_epochs, batch_ce_loss / update_epochs, raw_group_rewards.mean().item(), avg_components


# ---- validation (omr_grpo_train.py:456-492) -----------------------------------------------------------------------------------------------
def validation_loop(dataloader, policy_theta, reward_config, rollout_config, ce_loss_fn, pad_idx, device, *, reward_fn=None, slots=None,
                    uniforms_fn=None, autocast_dtype=torch.bfloat16, grammar=None, loop_guard=None, logger=None):
    """Mini or full validation, depending on the dataloader: one sampled rollout per image (group size 1) at rollout_config's max_actions /
    top_k / temperature, scored by reward_fn, and the teacher-forced CE loss of each batch.  Returns (mean raw reward, mean RewardComponents,
    mean CE loss), each a mean over batches of per-batch means, as the reference computes them.

    The reference calls `policy_theta.forward_rollout_policy` here, a method it does not define (as in batch_policy_inference); the cached
    policy is what it means.  The rollouts go through cached_continuous_rollout_policy with `slots` decode rows (default: the cache's max
    batch size): a dataloader batch may be larger than the cache, and a rollout that never draws <eos> does not hold the others' rows to
    max_actions.  reward_fn: as grpo_update's (default make_token_reward_fn(reward_config, pad_idx): the token-level edit cost in the place
    of the reference's tree edit cost).  uniforms_fn(batch_index, R, max_actions) -> (R, max_actions) uniforms fixes the draws (default:
    torch's generator).  autocast_dtype: the reference validates under bf16 autocast; None runs without autocast.  grammar: a
    grammar.TokenAutomaton that constrains the rollouts and, with the default reward_fn, scores their well-formedness.  loop_guard with
    logger: the share of the rollouts a loops.LoopGuard's rule flags, a mean over batches like the rest, goes to
    `logger.log_loop_rate(rate, None)`; the rollouts are not guarded and what is returned does not change."""
    from ..loops import check_guard
    check_guard(loop_guard)
    validation_loop_rate = 0
    if reward_fn is None:
        reward_fn = make_token_reward_fn(reward_config, pad_idx, grammar=grammar)
    dev_type = torch.device(device).type
    num_batches = len(dataloader)
    validation_reward = 0
    validation_reward_components = RewardComponents(0, 0, 0, 0, 0)
    validation_ce_loss = 0
    group_size = 1
    with torch.no_grad(), torch.autocast(device_type=dev_type, dtype=autocast_dtype or torch.bfloat16, enabled=autocast_dtype is not None):
        for i, batch in enumerate(dataloader):
            imgs, target_lmx_seqs, _ = zip(*batch)
            imgs = [img.to(device, non_blocking=True) for img in imgs]
            target_lmx_seqs = [t.to(device, non_blocking=True) for t in target_lmx_seqs]
            img_latent, latent_attention_mask = policy_theta.encoder(imgs)
            img_latent = policy_theta.transition_head(img_latent)
            uniforms = uniforms_fn(i, len(imgs), rollout_config.max_actions) if uniforms_fn is not None else None
            if grammar is None:
                rollouts, _, rollout_mask = policy_theta.cached_continuous_rollout_policy(
                    img_latent, latent_attention_mask, rollout_config.max_actions, rollout_config.top_k, rollout_config.temperature, slots=slots,
                    group_size=group_size, uniforms=uniforms)
            else:
                rollouts, _, rollout_mask = policy_theta.cached_constrained_continuous_rollout_policy(
                    img_latent, latent_attention_mask, grammar, rollout_config.max_actions, rollout_config.top_k, rollout_config.temperature,
                    slots=slots, group_size=group_size, uniforms=uniforms)
            padded_targets = expand_target_lmx_seqs(target_lmx_seqs, group_size, pad_idx, device)
            got = reward_fn(rollouts, rollout_mask, padded_targets, batch)
            raw_rewards, reward_components = got if isinstance(got, tuple) else (got, None)
            validation_reward += raw_rewards.float().mean().item()
            if reward_components is not None:
                validation_reward_components += reward_components.avg_over_rollouts()
            if loop_guard is not None and logger is not None:
                validation_loop_rate = validation_loop_rate + loop_rate(rollouts, rollout_mask, loop_guard)
            validation_ce_loss += calc_teacher_forced_ce_loss(policy_theta, img_latent, latent_attention_mask, target_lmx_seqs, ce_loss_fn).item()
    if loop_guard is not None and logger is not None:
        logger.log_loop_rate(validation_loop_rate / num_batches, None)
    return validation_reward / num_batches, validation_reward_components / num_batches, validation_ce_loss / num_batches


def refresh_old_policy(old_policy, policy_theta):
    """The reference loop's refresh before each minibatch (omr_grpo_train.py:425-426): encoder and transition head are frozen, so only the decoder
    parameters are copied.  load_state_dict writes in place, which the decode engine's weight copies notice (parameter versions)."""
    old_policy.decoder.load_state_dict({k: v.clone() for k, v in policy_theta.decoder.state_dict().items()})

