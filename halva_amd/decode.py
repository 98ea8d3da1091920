"""KV-cached decoding (greedy, or temperature / top-k / top-p sampling) for LLaVA-1.5 (LlavaLlamaForCausalLM.generate) and VILA (VilaLlavaLlamaModel.generate) - forward only.

Stands in for the reference's HF `generate(..., use_cache=True)` decode path: the per-layer cache concat
(llava/model/language_model/modelling_llama.py:295-305) and the decode position rule `attention_mask.sum(1) - 1`
(llava/model/llava_arch.py:90-98) become halva_decode_rope_append, the single-query attention halva_decode_attn
(split-KV; include/halva_hip.h).  Everything else of a decode step is the training path's own pieces on [B, d] rows.

Cache layout, per layer: K, V bf16 [B, H, Lcap, D]; lens int32 [layers, B] on the device (each layer's append advances its own
row).  Prompts are right-padded: sequence b holds positions [0, seq_len[b]).

The functions below run on a DecodeStack (the Llama stack, the lm_head weight, whether the LoRA factors apply).  They also accept either
model wrapper, which hands over its own pieces through decode_stack(): LLaVA's `.model` / `.lm_head`, VILA's `.llm.model` /
`.llm.lm_head`.
"""
from collections import namedtuple

import torch

from . import kernels as K

DecodeStack = namedtuple("DecodeStack", "lm lm_head use_lora")
DecodeStack.__doc__ = "lm: halva_amd.llama.LlamaModel; lm_head: the [V, d] head weight; use_lora: apply the LoRA factors (unmerged)."


def _stack(model):
    return model if isinstance(model, DecodeStack) else model.decode_stack()


class KVCache:
    """[layers][K, V] bf16 [B, H, Lcap, D], lens int32 [layers, B] and the split-KV workspace, allocated once per generate call."""

    def __init__(self, model, B, Lcap, device=None):
        lm = _stack(model).lm
        cfg = lm.config
        dev = device or lm.embed_tokens.weight.device
        H = cfg.num_attention_heads
        D = cfg.hidden_size // H
        n = cfg.num_hidden_layers
        self.B, self.H, self.D, self.Lcap = B, H, D, Lcap
        self.k = [torch.empty(B, H, Lcap, D, dtype=torch.bfloat16, device=dev) for _ in range(n)]
        self.v = [torch.empty(B, H, Lcap, D, dtype=torch.bfloat16, device=dev) for _ in range(n)]
        self.lens = torch.zeros(n, B, dtype=torch.int32, device=dev)
        self.filled = 0            # host-side upper bound of max_b lens[b] (no device read): the next append goes to a slot below it + 1
        self.ws = torch.empty(max(K.decode_ws_bytes(B, H, Lcap), 16), dtype=torch.uint8, device=dev)
        # the append kernel takes the new token's position only through these rows (row p = position p, the linear RoPE scaling of
        # LlamaModel.rope already applied); they cover every slot of the cache
        cos, sin = lm.rope(Lcap, dev)
        if cos.shape[0] < Lcap:
            lm._rope = {}
            cos, sin = lm.rope(Lcap, dev)
        self.cos, self.sin = cos, sin

    def fill(self, layer_idx, qkv, seq_len):
        """Prompt pass: the rotated k and the plain v of the [B, T, 3*H*D] projection into slots [0, T) (rows past seq_len[b] are
        written too and never read), lens = seq_len."""
        B, T = qkv.shape[0], qkv.shape[1]
        if T > self.Lcap:
            raise ValueError("prompt of %d rows does not fit a cache of %d slots" % (T, self.Lcap))
        kv = qkv.view(B, T, 3, self.H, self.D)
        self.k[layer_idx][:, :, :T].copy_(kv[:, :, 1].transpose(1, 2))
        self.v[layer_idx][:, :, :T].copy_(kv[:, :, 2].transpose(1, 2))
        self.lens[layer_idx].copy_(seq_len)
        self.filled = T


def _lm_head(st, h):
    return torch.nn.functional.linear(h, st.lm_head).float()


@torch.no_grad()
def prefill(model, inputs_embeds, seq_len, cache):
    """The prompt pass: run_layers on right-padded inputs_embeds [B, T, d] (sequence b = rows [0, seq_len[b])) with the cache fill
    hooked into every layer; the top layer runs only the last prompt row of each sequence.  -> last-row logits [B, V] fp32."""
    st = _stack(model)
    B, T, _ = inputs_embeds.shape
    dev = inputs_embeds.device
    seq_len = torch.as_tensor(seq_len, dtype=torch.int32)
    if int(seq_len.min()) < 1 or int(seq_len.max()) > T:
        raise ValueError("every prompt needs between 1 and T=%d rows" % T)
    seq_len_d = seq_len.to(dev)
    rows = (torch.arange(B, dtype=torch.int64) * T + seq_len.long() - 1).to(dev)
    h = st.lm.run_layers(inputs_embeds.to(torch.bfloat16), torch.zeros(B, dtype=torch.int32, device=dev), seq_len_d, st.use_lora, None,
                         rows, kv_hook=lambda i, qkv: cache.fill(i, qkv, seq_len_d))
    return _lm_head(st, h)


@torch.no_grad()
def decode_step(model, cache, token_ids):
    """One new token per sequence: token_ids [B] -> logits [B, V] fp32.  Appends each layer's k / v at slot lens[b]."""
    if cache.filled >= min(cache.Lcap, cache.cos.shape[0]):
        # the append kernel leaves a full cache untouched (it never writes out of bounds): refuse here instead of attending without
        # the new token
        raise RuntimeError("KV cache full: %d slots used of %d; allocate the cache for the prompt plus every new token" % (cache.filled, cache.Lcap))
    cache.filled += 1
    st = _stack(model)
    lm = st.lm
    x = lm.embed_tokens(token_ids.to(lm.embed_tokens.weight.device).long())          # a fresh buffer: the residual adds run on it in place
    for i, layer in enumerate(lm.layers):
        x = layer.decode(x, cache, i, st.use_lora)
    return _lm_head(st, lm.norm(x))


# ------------------------------------------------------------------------------------------------
# the generation loop shared by both generate() methods: greedy, or temperature / top-k / top-p sampling
def check_generate_args(num_beams, do_sample, max_new_tokens, temperature=None, top_k=None, top_p=None):
    """The calls the reference's hallucination benchmarks make: do_sample=False (greedy; temperature and top_p are ignored, as HF ignores
    them) or do_sample=True with a temperature, both with num_beams=1.  -> None for greedy, (temperature, top_k, top_p) for sampling with
    HF's GenerationConfig defaults filled in: top_k None = 50 (0 = off), top_p None = 1.0."""
    if num_beams is not None and num_beams > 1:
        raise NotImplementedError("generate: beam search (num_beams=%d) is not implemented; greedy decoding and sampling only" % num_beams)
    if max_new_tokens is None or max_new_tokens < 1:
        raise ValueError("max_new_tokens must be >= 1")
    if not do_sample:
        return None
    if temperature is None:
        raise NotImplementedError("generate: sampling (do_sample=True) needs an explicit temperature: the model carries no "
                                  "generation_config whose defaults could apply")
    temperature, top_k, top_p = float(temperature), 50 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p)
    if not (temperature > 0 and temperature != float("inf")):
        raise ValueError("generate: temperature=%r (sampling needs a finite temperature > 0; do_sample=False decodes greedily)" % temperature)
    if not 0 < top_p <= 1:
        raise ValueError("generate: top_p=%r (needs 0 < top_p <= 1)" % top_p)
    if top_k < 0:
        raise ValueError("generate: top_k=%r (needs >= 0; 0 turns the cut off)" % top_k)
    return temperature, top_k, top_p


def eos_and_pad(config, eos_token_id, pad_token_id, device):
    """-> (EOS ids as a LongTensor, pad id).  EOS: eos_token_id, else config.eos_token_id (an int or a list; [] = none).  Pad:
    pad_token_id, else config.pad_token_id, else the first EOS id, else 0."""
    eos = config.eos_token_id if eos_token_id is None else eos_token_id
    eos_ids = torch.as_tensor([] if eos is None else ([eos] if isinstance(eos, int) else list(eos)), dtype=torch.long, device=device)
    pad = pad_token_id if pad_token_id is not None else getattr(config, "pad_token_id", None)
    pad = pad if pad is not None else (int(eos_ids[0]) if eos_ids.numel() else 0)
    return eos_ids, pad


def _generate_loop(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, select, stopping_criteria, prefix):
    """Prefill, then select -> decode_step until every row is done or after max_new_tokens steps -> LongTensor [B, n] of new tokens.
    select(logits [B, V] fp32) -> (next tokens [B], None) or (next tokens [B], bool [B] of rows it could not serve); with the latter the
    flags ride on the step's one host sync and a set flag of a live row raises."""
    dev = inputs_embeds.device
    B = inputs_embeds.shape[0]
    crits = [] if stopping_criteria is None else ([stopping_criteria] if callable(stopping_criteria) else list(stopping_criteria))
    cache = KVCache(model, B, inputs_embeds.shape[1] + max_new_tokens, dev)
    logits = prefill(model, inputs_embeds, seq_len, cache)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    out = []
    for step in range(max_new_tokens):
        nxt, bad = select(logits)
        if bad is not None:
            bad = bad & ~done
        nxt = torch.where(done, torch.full_like(nxt, pad), nxt)
        out.append(nxt)
        if eos_ids.numel():
            done = done | torch.isin(nxt, eos_ids)
        if crits:
            seq = torch.stack(out, 1) if prefix is None else torch.cat([prefix, torch.stack(out, 1)], 1)
            for crit in crits:
                stop = crit(seq, logits)
                if isinstance(stop, torch.Tensor):
                    done = done | stop.to(dev, torch.bool).view(-1).expand(B)
                elif stop:
                    done = torch.ones_like(done)
        if bad is None:
            if step + 1 == max_new_tokens or bool(done.all()):          # the step's one host sync
                break
        else:
            flags = torch.cat([done.all().view(1), bad]).tolist()       # the step's one host sync
            if any(flags[1:]):
                raise RuntimeError("generate: row %d has no token to sample at step %d (NaN or inf logits, or none above -inf)"
                                   % (flags[1:].index(True), step))
            if step + 1 == max_new_tokens or flags[0]:
                break
        logits = decode_step(model, cache, nxt)
    return torch.stack(out, 1)


@torch.no_grad()
def greedy(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, stopping_criteria=None, prefix=None):
    """Prefill, then argmax -> decode_step until every row is done or after max_new_tokens steps -> LongTensor [B, n] of new tokens.

    A row that emitted an id of eos_ids is done and gets `pad` from then on.  stopping_criteria: a callable or a list of them (HF
    StoppingCriteriaList semantics: any criterion that returns True stops the batch; a tensor it returns marks rows done), each called
    after every step as criterion(seq, logits) with seq = cat(prefix, new tokens), or the new tokens alone when prefix is None.
    One host sync per step."""
    return _generate_loop(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, lambda logits: (logits.argmax(-1), None),
                          stopping_criteria, prefix)


@torch.no_grad()
def sample(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, temperature, top_k, top_p, generator=None, stopping_criteria=None,
           prefix=None):
    """As greedy(), with each step's token drawn from the temperature / top-k / top-p distribution of its logits by ONE native launch
    (kernels.sample_top_k_top_p; top_k 0 = off, top_p 1 = off).  Each step draws u = torch.rand(B, generator=generator) on the device
    exactly once, done rows included, so a row's stream does not depend on when other rows finish.  A live row whose logits leave nothing
    to sample (NaN, inf) raises RuntimeError; the flag rides on the step's one host sync."""
    dev = inputs_embeds.device
    B = inputs_embeds.shape[0]
    V = _stack(model).lm_head.shape[0]
    if V > K.sample_max_vocab():
        raise ValueError("generate: sampling takes a vocabulary of at most %d entries, the head has %d" % (K.sample_max_vocab(), V))

    def select(logits):
        u = torch.rand(B, device=dev, generator=generator)
        tok = K.sample_top_k_top_p(logits, u, temperature, top_k, top_p)
        return tok, tok < 0
    return _generate_loop(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, select, stopping_criteria, prefix)
