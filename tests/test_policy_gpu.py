"""GPU tests of GRPO training on the toy goldens: LlavaEngine.forward(policy=) / token_logps, the model's policy_loss / token_logps and
GRPOTrainer.  The anchors are bit for bit: with advantages 1, weights 1 / count, no old or reference log-probs and beta 0 the step is
the SFT step; old log-probs taken by token_logps give ratio exactly 1; zero advantages give zero gradients; a seeded run repeats."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from radvlm_amd.policy import sample_seeds
from radvlm_amd.splice import shifted_labels
from test_generate_gpu import CASES, _load, _model, _prompt

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _batch(g, images, sizes):
    return dict(input_ids=g["input_ids"], attention_mask=g["attention_mask"], labels=g["labels"], images=images, image_sizes=sizes)


def _grads(model, run):
    """The flat gradient buffer after one forward + backward from a clean accumulator."""
    eng = model.engine
    eng.zero_grad()
    out = run()
    out.loss.backward()
    torch.cuda.synchronize()
    return eng.grads.clone(), out


def _counts(model, batch):
    """Scored tokens per sample, from the spliced labels."""
    plan = model.engine.plan(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["images"], batch["image_sizes"])
    return (shifted_labels(plan["labels"]) != -100).sum(1)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_sft_anchor_padded_packed_and_head_rows(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw).train()
    batch = _batch(g, images, sizes)
    count = int(_counts(model, batch).sum())
    B = g["input_ids"].shape[0]
    for packed in (False, True):
        for head_rows in ("labeled", "all"):
            model.engine.packed, model.engine.head_rows = packed, head_rows
            sft, out_sft = _grads(model, lambda: model(**batch))
            assert float(sft.float().abs().max()) > 0
            for weights in (None, [1.0 / count] * B):
                pol, out = _grads(model, lambda: model.policy_loss(**batch, advantages=[1.0] * B, weights=weights))
                assert torch.equal(_bits(pol), _bits(sft)), (case, packed, head_rows, weights is None)
                assert out.stats["n_scored"] == count and float(out.clip.abs().max()) == 0.0 and float(out.kl.abs().max()) == 0.0
                # the VALUE of the surrogate at r = 1 is -A per token (only its gradient is the cross entropy's): sum(w * -1) = -1
                assert abs(float(out.loss.detach()) + 1.0) <= count * 2.0 ** -23
                # ... and -mean(logp) is the cross entropy, summed in another order
                assert abs(-float(out.logps.double().sum()) / count - float(out_sft.loss.detach())) <= count * 2.0 ** -23 * float(out.logps.abs().sum()) / count


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_token_logps_count_order_and_loss(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw).train()
    eng = model.engine
    batch = _batch(g, images, sizes)
    counts = _counts(model, batch)
    n = int(counts.sum())
    loss = float(model(**batch).loss.detach())
    eng.ctx = None
    lp = model.token_logps(**batch)
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (n,) and eng.ctx is None
    assert eng.last_policy["scored"].tolist() == counts.tolist()
    assert abs(-float(lp.double().sum()) / n - loss) <= n * 2.0 ** -23 * float(lp.abs().sum()) / n
    # scored order: sample by sample, positions ascending -- against the fp32 logits of the all-rows head (head_rows = "all"), which are
    # the accumulators the bf16 logits of that same product are rounded from: each bf16 logit lies within 2^-9 |z| of its fp32 value, so
    # a token's logp moves by at most 2 * 2^-9 max|z| (its target and the lse)
    eng.packed, eng.head_rows = False, "all"
    eng.forward(batch["input_ids"], batch["attention_mask"], batch["labels"], images, image_sizes=sizes, want_logits=True)
    logits = eng.last_logits.double().cpu()
    eng.ctx = None
    tgt = shifted_labels(eng.plan(batch["input_ids"], batch["attention_mask"], batch["labels"], images, sizes)["labels"])
    b, s = np.nonzero(tgt != -100)
    ref = torch.log_softmax(logits[b, s], -1)[torch.arange(n), torch.from_numpy(tgt[b, s])]
    bound = 2 * 2.0 ** -9 * float(logits[b, s].abs().max()) + 1e-6
    err = float((model.token_logps(**batch).double().cpu() - ref).abs().max())
    print(f"token_logps against the fp32 logits: max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    # the labelled-rows head, padded and packed, scores the same tokens in the same order (its accuracy is the parity tests' subject; an
    # order mix-up would decorrelate the two, as the shuffled reference shows)
    corr = lambda x: float(torch.corrcoef(torch.stack([x.double().cpu(), ref]))[0, 1])
    assert corr(ref[torch.randperm(n, generator=torch.Generator().manual_seed(0))]) < 0.9
    for packed in (False, True):
        eng.packed, eng.head_rows = packed, "labeled"
        got = model.token_logps(**batch)
        assert tuple(got.shape) == (n,) and corr(got) > 0.99, (packed, corr(got))


def test_old_logps_from_token_logps_give_ratio_one(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw).train()
    batch = _batch(g, images, sizes)
    adv = [0.7, -1.3, 0.4]
    on_policy, _ = _grads(model, lambda: model.policy_loss(**batch, advantages=adv))
    old = model.token_logps(**batch)
    with_old, out = _grads(model, lambda: model.policy_loss(**batch, advantages=adv, old_logps=old, epsilon=0.2, epsilon_high=0.28))
    assert torch.equal(_bits(with_old), _bits(on_policy)) and float(on_policy.float().abs().max()) > 0
    assert float(out.clip.abs().max()) == 0.0 and torch.equal(_bits(out.logps), _bits(old))
    assert not bool(model.engine.last_policy["ratio_one"].any())
    # a reference equal to the policy: kl exactly 0 and no KL gradient
    with_ref, out = _grads(model, lambda: model.policy_loss(**batch, advantages=adv, old_logps=old, ref_logps=old, beta=0.04))
    assert torch.equal(_bits(with_ref), _bits(on_policy)) and float(out.kl.abs().max()) == 0.0
    # old log-probs half a nat lower: r = e^0.5 > 1 + eps, so positive-advantage samples clip high and the negative one stays active
    counts = _counts(model, batch)
    _, out = _grads(model, lambda: model.policy_loss(**batch, advantages=adv, old_logps=old - 0.5))
    want = np.repeat(np.array([2.0, 0.0, 2.0]), counts)
    assert out.clip.cpu().tolist() == want.tolist()
    assert float(out.stats["clip_ratio/high"]) == pytest.approx((want == 2).mean()) and float(out.stats["clip_ratio/low"]) == 0.0


def test_zero_advantages_and_shape_errors(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw).train()
    batch = _batch(g, images, sizes)
    counts = _counts(model, batch)
    model.engine.grads.fill_(1.0)
    zero, out = _grads(model, lambda: model.policy_loss(**batch, advantages=[0.0, 0.0, 0.0]))
    assert float(zero.float().abs().max()) == 0.0 and float(out.loss.detach()) == 0.0
    per_token = [np.ones(int(c)) for c in counts]
    short = per_token[:-1] + [per_token[-1][:-1]]
    with pytest.raises(ValueError, match=f"sample {len(counts) - 1}"):
        model.policy_loss(**batch, advantages=short)
    with pytest.raises(ValueError, match=f"weights.*sample {len(counts) - 1}"):
        model.policy_loss(**batch, advantages=per_token, weights=np.ones(int(counts.sum()) - 1))
    with pytest.raises(ValueError, match="ref_logps"):
        model.policy_loss(**batch, advantages=per_token, beta=0.1)
    # per-token arrays, as a list and as their concatenation, are the per-sample floats spelled out
    a, _ = _grads(model, lambda: model.policy_loss(**batch, advantages=[0.5, -1.0, 2.0]))
    b, _ = _grads(model, lambda: model.policy_loss(**batch, advantages=[0.5 * per_token[0], -1.0 * per_token[1], 2.0 * per_token[2]]))
    c, _ = _grads(model, lambda: model.policy_loss(**batch, advantages=np.repeat([0.5, -1.0, 2.0], counts)))
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))


# ------------------------------------------------------------------------------------------------ the trainer
def _even_fraction(completion_ids, **_):
    return [float(np.mean([t % 2 == 0 for t in c])) if len(c) else 0.0 for c in completion_ids]


def _dataset(g, images, sizes, n=2):
    return [dict(prompt_ids=_prompt(g, b), images=images[b], image_sizes=sizes[b], tag=f"p{b}") for b in range(n)]


def _args(**kw):
    base = dict(per_device_train_batch_size=2, num_generations=4, max_completion_length=6, max_steps=2, learning_rate=1e-3, weight_decay=0.0,
                lr_scheduler_type="constant", seed=11, log_completions=True, max_grad_norm=1.0)
    return SimpleNamespace(**dict(base, **kw))


def _strip_times(log):
    return [{k: v for k, v in rec.items() if not k.startswith("time/")} for rec in log]


def test_trainer_runs_repeat_bit_for_bit(golden_dir):
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    g, images, sizes, kw = _load(golden_dir, "toy")
    data = _dataset(g, images, sizes)
    seen = []

    def reward(prompts, completions, completion_ids, tag, **_):
        seen.append((len(prompts), completions == completion_ids, tag))
        return _even_fraction(completion_ids)

    runs = []
    for r in range(2):
        model = _model("toy", kw).train()
        eng = model.engine
        alone = None
        if r == 1:      # what generate_batch alone returns for step 1's requests (it leaves the training state untouched)
            order = [int(seen[0][2][p * 4][1:]) for p in range(2)]          # the prompts of step 1 in the epoch's seeded order
            out = model.generate_batch([data[b]["prompt_ids"] for b in order for _ in range(4)], images=[data[b]["images"] for b in order for _ in range(4)],
                                       image_sizes=[data[b]["image_sizes"] for b in order for _ in range(4)], do_sample=True,
                                       seed=sample_seeds(11, 0, 2, 4), share_prefix=True, max_new_tokens=6, top_k=None)    # the trainer's default: no top-k
            alone = [out[f"req_{i}"].generated_tokens for i in range(8)]
        v0, w0 = eng.weights_version, eng.lm.flat.clone()
        state = GRPOTrainer(model, _args(), data, reward).train()
        torch.cuda.synchronize()
        assert eng.weights_version >= v0 + 2 and not torch.equal(_bits(eng.lm.flat), _bits(w0)) and eng.loss_scale == 1.0
        runs.append((eng.lm.flat.clone(), _strip_times(state["log_history"]), alone))
    (wa, la, _), (wb, lb, alone) = runs
    assert torch.equal(_bits(wa), _bits(wb)) and la == lb and len(la) == 2
    assert la[0]["completion_ids"] == alone and la[0]["completion_ids"] != la[1]["completion_ids"]
    assert all(n == 8 and same for n, same, _ in seen) and all(t[0] == t[1] == t[2] == t[3] and t[4] == t[7] for _, _, t in seen)
    for rec in la:
        assert set(rec) >= {"reward", "reward_std", "frac_reward_zero_std", "completions/mean_length", "clip_ratio/low", "clip_ratio/high", "kl",
                            "loss", "grad_norm", "learning_rate", "step"}
        assert rec["clip_ratio/low"] == rec["clip_ratio/high"] == rec["kl"] == 0.0 and 0.0 <= rec["reward"] <= 1.0
        assert 1 <= rec["completions/mean_length"] <= 6 and rec["grad_norm"] is not None


def test_trainer_constant_rewards_leave_the_weights(golden_dir):
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw).train()
    data = _dataset(g, images, sizes) + [dict(prompt_ids=np.array([5, 17, 33, 2, 9], dtype=np.int64), tag="text")]     # one text-only prompt
    w0 = model.engine.lm.flat.clone()
    constant_in_group = lambda prompts, completion_ids, tag, **_: [float(len(t)) for t in tag]
    state = GRPOTrainer(model, _args(per_device_train_batch_size=3, max_steps=1, gradient_accumulation_steps=2), data, constant_in_group).train()
    torch.cuda.synchronize()
    assert torch.equal(_bits(model.engine.lm.flat), _bits(w0)) and model.engine.weights_version > 0
    rec = state["log_history"][0]
    assert rec["frac_reward_zero_std"] == 1.0 and rec["reward_std"] == 0.0 and rec["loss"] == 0.0 and rec["grad_norm"] == 0.0


def test_trainer_iterations_and_reference_model(golden_dir):
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model, ref = _model("toy_qwen", kw).train(), _model("toy_qwen", kw)
    state = GRPOTrainer(model, _args(max_steps=1, num_iterations=2, beta=0.04, loss_type="grpo", learning_rate=3e-3), _dataset(g, images, sizes),
                        [_even_fraction, lambda completion_ids, **_: [0.0] * len(completion_ids)], ref_model=ref, reward_weights=[1.0, 5.0]).train()
    first, second = state["log_history"][0]["iterations"]
    assert first["clip_ratio/low"] == first["clip_ratio/high"] == 0.0 and first["kl"] == 0.0       # ratio exactly 1, reference == policy
    assert second["kl"] > 0.0 and 0.0 <= second["clip_ratio/low"] <= 1.0 and 0.0 <= second["clip_ratio/high"] <= 1.0
    assert model.engine.opt_step == 2 and ref.engine.opt_step == 0


def test_trainer_refusals(golden_dir):
    from radvlm_amd.config import GEOMETRIES
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    data = _dataset(g, images, sizes)
    with pytest.raises(ValueError, match="num_generations"):
        GRPOTrainer(model, _args(num_generations=1), data, _even_fraction)
    with pytest.raises(ValueError, match="ref_model"):
        GRPOTrainer(model, _args(beta=0.04), data, _even_fraction)
    with pytest.raises(ValueError):
        GRPOTrainer(model, _args(loss_type="sum"), data, _even_fraction)
    with pytest.raises(ValueError):
        GRPOTrainer(model, _args(), data, [_even_fraction], reward_weights=[1.0, 2.0])
    lora = LlavaLlamaForCausalLM(LlavaConfig(geometry=GEOMETRIES["toy"], lora=dict(r=8, alpha=16, dropout=0.0)), device="cuda:0", init="portable", seed=0)
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        GRPOTrainer(lora, _args(), data, _even_fraction)
    with pytest.raises(NotImplementedError):
        model.eval()(input_ids=g["input_ids"], attention_mask=g["attention_mask"], labels=g["labels"], images=images, dpo_forward=True)
