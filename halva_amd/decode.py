"""KV-cached decoding (greedy, temperature / top-k / top-p sampling, or either of them contrastively against a second prompt) for LLaVA-1.5 (LlavaLlamaForCausalLM.generate) and VILA (VilaLlavaLlamaModel.generate) - forward only.

Stands in for the reference's HF `generate(..., use_cache=True)` decode path: the per-layer cache concat
(llava/model/language_model/modelling_llama.py:295-305) and the decode position rule `attention_mask.sum(1) - 1`
(llava/model/llava_arch.py:90-98) become halva_decode_rope_append, the single-query attention halva_decode_attn
(split-KV; include/halva_hip.h).  Everything else of a decode step is the training path's own pieces on [B, d] rows.

Cache layout, per layer: K, V bf16 [B, H, Lcap, D]; lens int32 [layers, B] on the device (each layer's append advances its own
row).  Prompts are right-padded: sequence b holds positions [0, seq_len[b]).

A ForkCache gives M members the rows of a parent cache as a shared prefix, read in place, and own rows behind them (n sampled answers to one
prompt, many questions about one image): K, V bf16 [M, H, Lown, D], own_lens int32 [layers, M], prefix_lens int32 [P] as recorded at fork time.

A BeamCache is the ForkCache of beam search (B prompts x K beams, member b * K + i): beside the own rows it keeps an ancestry table anc
int32 [2, M, Lown], one pair for all layers - anc[cur][m][t] is the member whose own slot t holds row t of member m's history - so that a
beam that continues another beam's history moves no K / V row.

The three caches share one surface, and nothing above them asks which one it holds: rows (sequences or members), room (rows a member can
hold), Lcap, lens, filled, full_step (decode_step's message on a full cache), rows_refusal (why extend() is refused, or None),
attend_step(layer, qkv, H, D, out_width) - RoPE + append of one new row per member, then the single-query attention - and
attend_rows(layer, qkv, n_new_d, H, D, out_width) - append, attention and advance of up to n rows per member.  decode_step() and extend() are
written once over it; DecoderLayer.decode / .extend hand the projection to it.

The functions below run on a DecodeStack (the Llama stack, the lm_head weight, whether the LoRA factors apply).  They also accept either
model wrapper, which hands over its own pieces through decode_stack(): LLaVA's `.model` / `.lm_head`, VILA's `.llm.model` /
`.llm.lm_head`.
"""
from collections import namedtuple

import torch

from . import kernels as K
from .beam import BeamOutput, BeamState, check_beam_args

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
        self.rope = lm.rope        # (a ForkCache whose positions outgrow cos / sin re-sizes them through it)
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

    full_step = "KV cache full: %d slots used of %d; allocate the cache for the prompt plus every new token"
    rows_refusal = None
    rows = property(lambda self: self.B)
    room = property(lambda self: min(self.Lcap, self.cos.shape[0]))

    def attend_step(self, layer_idx, qkv, H, D, out_width):
        kc, vc, lens = self.k[layer_idx], self.v[layer_idx], self.lens[layer_idx]
        K.decode_rope_append(qkv, self.cos, self.sin, kc, vc, lens, H, D)
        return K.decode_attention(qkv, kc, vc, lens, self.ws, H, D, out_width)

    def attend_rows(self, layer_idx, qkv, n_new_d, H, D, out_width):
        kc, vc, lens = self.k[layer_idx], self.v[layer_idx], self.lens[layer_idx]
        K.extend_rope_append(qkv, self.cos, self.sin, kc, vc, lens, n_new_d, H, D)
        a = K.extend_attention(qkv, kc, vc, lens, n_new_d, None, H, D, out_width)      # (its workspace is empty by design)
        K.extend_advance(lens, n_new_d, self.Lcap)
        return a

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


def _check_room(cache):
    if cache.filled >= cache.room:
        # the append kernels leave a full cache untouched (they never write out of bounds): refuse here instead of attending without the
        # new token
        raise RuntimeError(cache.full_step % (cache.filled, cache.Lcap))


@torch.no_grad()
def decode_step(model, cache, token_ids):
    """One new token per sequence of a KVCache, or per member of a ForkCache / BeamCache: token_ids [rows] -> logits [rows, V] fp32.  Each
    layer appends its k / v behind the rows the member holds (cache.attend_step)."""
    _check_room(cache)
    cache.filled += 1
    st = _stack(model)
    lm = st.lm
    x = lm.embed_tokens(token_ids.to(lm.embed_tokens.weight.device).long())          # a fresh buffer: the residual adds run on it in place
    x = lm.each_layer(x, None, lambda i, layer, x, top: (layer.decode(x, cache, i, st.use_lora), None))
    return _lm_head(st, x)


@torch.no_grad()
def extend(model, cache, inputs_embeds, n_new):
    """Several new rows per sequence (or member of a ForkCache) in one pass over a cache that already holds rows: inputs_embeds [B, n, d],
    n_new [B] host ints with 0 <= n_new[b] <= n (sequence b pushes its rows [0, n_new[b]) behind the rows it holds) -> logits [B, V] fp32
    of each sequence's last new row.  A sequence with n_new[b] == 0 is left as it is (cache and lens untouched) and gets NaN logits:
    callers mask them.  Every check runs before the first launch; a block that does not fit raises RuntimeError like decode_step's."""
    if cache.rows_refusal:
        raise NotImplementedError(cache.rows_refusal)
    st = _stack(model)
    lm = st.lm
    B = cache.rows
    if inputs_embeds.ndim != 3 or inputs_embeds.shape[0] != B:
        raise ValueError("extend needs inputs_embeds [B=%d, n, d], got %s" % (B, tuple(inputs_embeds.shape)))
    n = inputs_embeds.shape[1]
    n_new = torch.as_tensor(n_new, dtype=torch.int32).view(-1).cpu()
    if n_new.numel() != B:
        raise ValueError("extend needs one n_new per sequence (%d), got %d" % (B, n_new.numel()))
    most = int(n_new.max())
    if most < 1 or int(n_new.min()) < 0 or most > n:
        raise ValueError("extend: every n_new[b] must lie in [0, n=%d] and one of them must be >= 1, got %s" % (n, n_new.tolist()))
    if cache.filled + most > cache.room:
        raise RuntimeError("KV cache full: %d slots used of %d, %d more asked for; allocate the cache for the prompt plus every new row"
                           % (cache.filled, cache.Lcap, most))
    cache.filled += most
    dev = lm.embed_tokens.weight.device
    n_new_d = n_new.to(dev)
    rows = (torch.arange(B, dtype=torch.int64) * n + (n_new.long() - 1).clamp_(min=0)).to(dev)
    x = inputs_embeds.to(dev, torch.bfloat16, copy=True).contiguous()      # a buffer of our own: the residual adds run on it in place
    x = lm.each_layer(x, rows, lambda i, layer, x, top: (layer.extend(x, cache, i, n_new_d, st.use_lora, top), None))
    return _lm_head(st, x).masked_fill_((n_new_d == 0)[:, None], float("nan"))


def chunk_schedule(seq_len, T, chunk):
    """How prefill_chunked cuts right-padded prompts of seq_len[b] rows (T columns) into blocks of `chunk` rows: a list of
    (first column, columns, n_new [B]).  Block 0 is the prefill() call (n_new = seq_len clipped to its columns); blocks that hold only
    padding are dropped."""
    seq_len = [int(v) for v in seq_len]
    if chunk is None or int(chunk) < 1:
        raise ValueError("prefill_chunk must be an int >= 1, got %r" % (chunk,))
    chunk = int(chunk)
    out, done = [], 0
    while done < max(seq_len) or not out:
        n = min(chunk, T - done)
        out.append((done, n, [min(max(v - done, 0), n) for v in seq_len]))
        done += n
    return out


@torch.no_grad()
def prefill_chunked(model, inputs_embeds, seq_len, cache, chunk):
    """prefill() in blocks of `chunk` rows, so that no pass holds more than [B, chunk, .] activations: the first block through prefill(),
    the others through extend() over the rows the cache already holds.  -> each sequence's last-prompt-row logits [B, V] fp32, taken from
    the block in which that sequence ended."""
    B, T, _ = inputs_embeds.shape
    seq_len = torch.as_tensor(seq_len, dtype=torch.int32).cpu()
    if int(seq_len.min()) < 1 or int(seq_len.max()) > T:
        raise ValueError("every prompt needs between 1 and T=%d rows" % T)
    logits = None
    for start, n, n_new in chunk_schedule(seq_len.tolist(), T, chunk):
        block = inputs_embeds[:, start:start + n].contiguous()
        if start == 0:
            logits = prefill(model, block, torch.tensor(n_new, dtype=torch.int32), cache)
            cache.filled = max(n_new)          # (fill() counts the block's columns; nothing beyond the longest prompt's rows is ever read)
        else:
            lg = extend(model, cache, block, n_new)
            live = torch.tensor([v > 0 for v in n_new], device=lg.device)
            logits = torch.where(live[:, None], lg, logits)
    return logits


def prompt_pass(model, inputs_embeds, seq_len, cache, prefill_chunk=None):
    """prefill(), or prefill_chunked() in blocks of prefill_chunk rows when one is given."""
    if prefill_chunk is None:
        return prefill(model, inputs_embeds, seq_len, cache)
    return prefill_chunked(model, inputs_embeds, seq_len, cache, prefill_chunk)


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


def _generate_loop(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, select, stopping_criteria, prefix, prefill_chunk=None):
    """Prefill, then select -> decode_step until every row is done or after max_new_tokens steps -> LongTensor [B, n] of new tokens.
    select(logits [B, V] fp32) -> (next tokens [B], None) or (next tokens [B], bool [B] of rows it could not serve); with the latter the
    flags ride on the step's one host sync and a set flag of a live row raises.  prefill_chunk: as prompt_pass()."""
    B = inputs_embeds.shape[0]
    cache = KVCache(model, B, inputs_embeds.shape[1] + max_new_tokens, inputs_embeds.device)
    logits = prompt_pass(model, inputs_embeds, seq_len, cache, prefill_chunk)
    return _loop_from(model, cache, logits, max_new_tokens, eos_ids, pad, select, stopping_criteria, prefix)[0]


def _loop_from(model, cache, logits, max_new_tokens, eos_ids, pad, select, stopping_criteria, prefix):
    """_generate_loop's steps from a given (cache, logits [B, V]) -> (new tokens [B, n], real [B] on the device: how many of a row's n
    tokens it selected while live, the others being pad).  The last selected token is not pushed through the model.  cache: any of the
    three (a ForkCache's rows are its members)."""
    dev = logits.device
    B = logits.shape[0]
    crits = [] if stopping_criteria is None else ([stopping_criteria] if callable(stopping_criteria) else list(stopping_criteria))
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    real = torch.zeros(B, dtype=torch.int64, device=dev)
    out = []
    for step in range(max_new_tokens):
        nxt, bad = select(logits)
        real = real + ~done
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
    return torch.stack(out, 1), real


def _argmax(logits):
    return logits.argmax(-1), None


@torch.no_grad()
def greedy(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, stopping_criteria=None, prefix=None, prefill_chunk=None):
    """Prefill, then argmax -> decode_step until every row is done or after max_new_tokens steps -> LongTensor [B, n] of new tokens.

    A row that emitted an id of eos_ids is done and gets `pad` from then on.  stopping_criteria: a callable or a list of them (HF
    StoppingCriteriaList semantics: any criterion that returns True stops the batch; a tensor it returns marks rows done), each called
    after every step as criterion(seq, logits) with seq = cat(prefix, new tokens), or the new tokens alone when prefix is None.
    One host sync per step."""
    return _generate_loop(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, _argmax, stopping_criteria, prefix, prefill_chunk)


@torch.no_grad()
def sample(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, temperature, top_k, top_p, generator=None, stopping_criteria=None,
           prefix=None, prefill_chunk=None):
    """As greedy(), with each step's token drawn from the temperature / top-k / top-p distribution of its logits by ONE native launch
    (kernels.sample_top_k_top_p; top_k 0 = off, top_p 1 = off).  Each step draws u = torch.rand(B, generator=generator) on the device
    exactly once, done rows included, so a row's stream does not depend on when other rows finish.  A live row whose logits leave nothing
    to sample (NaN, inf) raises RuntimeError; the flag rides on the step's one host sync."""
    select = _sampler(model, inputs_embeds.shape[0], inputs_embeds.device, temperature, top_k, top_p, generator)
    return _generate_loop(model, inputs_embeds, seq_len, max_new_tokens, eos_ids, pad, select, stopping_criteria, prefix, prefill_chunk)


def _sampler(model, B, dev, temperature, top_k, top_p, generator):
    """sample()'s select: one torch.rand(B) and one kernels.sample_top_k_top_p launch per step."""
    V = _stack(model).lm_head.shape[0]
    if V > K.sample_max_vocab():
        raise ValueError("generate: sampling takes a vocabulary of at most %d entries, the head has %d" % (K.sample_max_vocab(), V))

    def select(logits):
        u = torch.rand(B, device=dev, generator=generator)
        tok = K.sample_top_k_top_p(logits, u, temperature, top_k, top_p)
        return tok, tok < 0
    return select


def check_contrast_args(has_images_cd, has_negative_ids, has_negative_mask, cd_alpha, cd_beta, guidance_scale, num_beams, num_return_sequences):
    """generate's contrast arguments -> None when none of them is given (the call takes the plain path), else (alpha, beta) of
    contrast().  The contrast branch is images_cd (the same ids over other images) or negative_input_ids (another prompt), not both;
    cd_alpha (None = 0.5) >= 0 and 0 <= cd_beta (None = 0.1) <= 1 are VCD's, guidance_scale = g >= 1 is HF's alias for alpha = g - 1,
    beta = 0.  Every refusal is a ValueError and comes before any launch: contrast with num_beams > 1 or num_return_sequences > 1, a
    weight without a contrast branch (it would be ignored), both branches, both spellings of the weight."""
    weights = cd_alpha is not None or cd_beta is not None or guidance_scale is not None
    if not (has_images_cd or has_negative_ids):
        if weights or has_negative_mask:
            raise ValueError("generate: cd_alpha / cd_beta / guidance_scale / negative_attention_mask need a contrast branch: images_cd= or "
                             "negative_input_ids=")
        return None
    if has_images_cd and has_negative_ids:
        raise ValueError("generate: images_cd and negative_input_ids are two different contrast branches; give one of them")
    if has_negative_mask and not has_negative_ids:
        raise ValueError("generate: negative_attention_mask without negative_input_ids")
    if num_beams is not None and num_beams > 1:
        raise ValueError("generate: contrastive decoding with num_beams=%d is not supported; num_beams=1 only" % num_beams)
    if num_return_sequences is not None and int(num_return_sequences) != 1:
        raise ValueError("generate: contrastive decoding with num_return_sequences=%r is not supported; one sequence per prompt"
                         % (num_return_sequences,))
    if guidance_scale is not None:
        if cd_alpha is not None or cd_beta is not None:
            raise ValueError("generate: guidance_scale is an alias for cd_alpha = guidance_scale - 1, cd_beta = 0; give one spelling")
        g = float(guidance_scale)
        if not (g >= 1 and g != float("inf")):
            raise ValueError("generate: guidance_scale=%r (needs a finite value >= 1)" % (guidance_scale,))
        return g - 1.0, 0.0
    alpha, beta = 0.5 if cd_alpha is None else float(cd_alpha), 0.1 if cd_beta is None else float(cd_beta)
    if not (alpha >= 0 and alpha != float("inf")):
        raise ValueError("generate: cd_alpha=%r (needs a finite value >= 0)" % (cd_alpha,))
    if not 0 <= beta <= 1:
        raise ValueError("generate: cd_beta=%r (needs 0 <= cd_beta <= 1)" % (cd_beta,))
    return alpha, beta


@torch.no_grad()
def contrast(model, inputs_embeds, seq_len, embeds_cd, seq_len_cd, max_new_tokens, eos_ids, pad, alpha, beta, sampling=None, generator=None,
             stopping_criteria=None, prefix=None, prefill_chunk=None):
    """Contrastive decoding (VCD; classifier-free guidance with beta = 0): as greedy() / sample(), with each step's token chosen from
    (1 + alpha) * logits - alpha * logits_cd over the columns plausible under logits (kernels.contrast_select, ONE native launch) ->
    LongTensor [B, n].  The prompt as given (inputs_embeds [B, T, d], seq_len) and the contrast prompt (embeds_cd [B, T', d], seq_len_cd)
    share one KVCache of 2 B rows - rows [0, B) the former, rows [B, 2 B) the latter, right-padded to a common T - one prompt pass and one
    decode step per token: both rows of a pair push the same token.  sampling: None = greedy contrast (the lowest index among the maxima),
    or (temperature, top_k, top_p) with u = torch.rand(B, generator=generator) drawn exactly once per step, done rows included.
    stopping_criteria see the B rows of the prompt as given, with `prefix` in front."""
    B, T = inputs_embeds.shape[0], max(inputs_embeds.shape[1], embeds_cd.shape[1])
    if embeds_cd.shape[0] != B or embeds_cd.shape[2] != inputs_embeds.shape[2]:
        raise ValueError("contrast: the contrast prompt needs the prompt's batch and width %s, got %s"
                         % ((B, inputs_embeds.shape[2]), (embeds_cd.shape[0], embeds_cd.shape[2])))
    V = _stack(model).lm_head.shape[0]
    if V > K.sample_max_vocab():
        raise ValueError("generate: contrastive decoding takes a vocabulary of at most %d entries, the head has %d" % (K.sample_max_vocab(), V))
    dev = inputs_embeds.device
    both = torch.zeros(2 * B, T, inputs_embeds.shape[2], dtype=inputs_embeds.dtype, device=dev)
    both[:B, :inputs_embeds.shape[1]] = inputs_embeds
    both[B:, :embeds_cd.shape[1]] = embeds_cd.to(dev, inputs_embeds.dtype)
    lens = torch.cat([torch.as_tensor(seq_len, dtype=torch.int32).view(-1).cpu(), torch.as_tensor(seq_len_cd, dtype=torch.int32).view(-1).cpu()])
    temperature, top_k, top_p = (1.0, 1, 1.0) if sampling is None else sampling
    zeros = torch.zeros(B, dtype=torch.float32, device=dev)

    def select(logits):
        u = zeros if sampling is None else torch.rand(B, device=dev, generator=generator)
        tok = K.contrast_select(logits[:B], logits[B:], u, alpha, beta, temperature, top_k, top_p)
        return tok.repeat(2), (tok < 0).repeat(2)

    crits = [] if stopping_criteria is None else ([stopping_criteria] if callable(stopping_criteria) else list(stopping_criteria))

    def first_half(crit):
        def on_pairs(seq, logits):
            stop = crit(seq[:B] if prefix is None else torch.cat([prefix, seq[:B]], 1), logits[:B])
            return stop.to(dev, torch.bool).view(-1).expand(B).repeat(2) if isinstance(stop, torch.Tensor) else stop
        return on_pairs

    cache = KVCache(model, 2 * B, T + max_new_tokens, dev)
    logits = prompt_pass(model, both, lens, cache, prefill_chunk)
    out, _ = _loop_from(model, cache, logits, max_new_tokens, eos_ids, pad, select, [first_half(c) for c in crits] or None, None)
    return out[:B]


# ------------------------------------------------------------------------------------------------
class DecodeSession:
    """A KV cache kept alive between calls (LlavaLlamaForCausalLM.start_session / VilaLlavaLlamaModel.start_session): generate() continues
    from the kept last-row logits, append() pushes a text-only next turn through ONE extend() call.

    Per row the session keeps on the host: lens[b], the rows the cache holds, and pending[b], the tokens of the row's history that the
    cache does not hold yet - generate()'s loop ends without pushing its last selected token through the model.  A row that stopped (EOS, a
    stopping criterion) counts its tokens up to and including the one it stopped on; the pad tokens behind it belong to no history and are
    never kept: the loop's decode_step writes them behind the row's last real slot, and lens is set back to the host's count afterwards
    (slots at or beyond lens[b] are never read)."""

    def __init__(self, model, cache, logits, lens, config=None):
        self.model, self.cache, self.logits, self.config = model, cache, logits, config
        self.lens = [int(v) for v in lens]
        self.pending = [[] for _ in self.lens]
        self.max_len = cache.Lcap

    def _set_lens(self):
        cache = self.cache
        cache.lens.copy_(torch.tensor(self.lens, dtype=torch.int32).to(cache.lens.device).expand_as(cache.lens))
        cache.filled = max(self.lens)

    def _push(self, new):
        """pending[b] + new[b] of every row through one extend() call; the logits of a row's last new row replace its kept ones."""
        rows = [p + list(t) for p, t in zip(self.pending, new)]
        n_new = [len(r) for r in rows]
        n = max(n_new)
        if n == 0:
            return
        if max(self.lens) + n > self.max_len:
            raise RuntimeError("session full: %d rows held, %d more asked for, max_len=%d" % (max(self.lens), n, self.max_len))
        lm = _stack(self.model).lm
        dev = lm.embed_tokens.weight.device
        ids = torch.zeros(len(rows), n, dtype=torch.long)
        for b, r in enumerate(rows):
            ids[b, :len(r)] = torch.as_tensor(r, dtype=torch.long)
        lg = extend(self.model, self.cache, lm.embed_tokens(ids.to(dev)), n_new)
        live = torch.tensor([v > 0 for v in n_new], device=lg.device)
        self.logits = torch.where(live[:, None], lg, self.logits)
        self.lens = [a + b for a, b in zip(self.lens, n_new)]
        self.pending = [[] for _ in rows]
        self.cache.filled = max(self.lens)

    @torch.no_grad()
    def append(self, input_ids, attention_mask=None, images=None):
        """The next turn, text only: input_ids [B, m] right padded (attention_mask marks each row's ids).  Each row's pending tokens and
        then its new ids go through one extend() call, ragged.  Exceeding max_len raises RuntimeError before any launch."""
        if images is not None:
            raise NotImplementedError("session.append: images in a later turn are not implemented; start a new session")
        ids = torch.as_tensor(input_ids).detach().cpu().long()
        if ids.ndim != 2 or ids.shape[0] != len(self.lens):
            raise ValueError("session.append needs input_ids [B=%d, m]" % len(self.lens))
        if (ids < 0).any():
            raise NotImplementedError("session.append: image tokens in a later turn are not implemented")
        if attention_mask is None:
            new = [row.tolist() for row in ids]
        else:
            mask = torch.as_tensor(attention_mask).detach().cpu().bool()
            cnt = mask.sum(1).tolist()
            if any(not bool(mask[b, :c].all()) for b, c in enumerate(cnt)):
                raise NotImplementedError("session.append: left-padded or gapped rows are not supported; pad on the right")
            new = [ids[b, :c].tolist() for b, c in enumerate(cnt)]
        self._push(new)

    @torch.no_grad()
    def generate(self, max_new_tokens, do_sample=False, temperature=None, top_k=None, top_p=None, eos_token_id=None, pad_token_id=None,
                 stopping_criteria=None, generator=None):
        """_generate_loop's rules on the kept cache -> LongTensor [B, n] of the new tokens only (both model families).  Tokens a previous
        generate() left pending are pushed first."""
        sampling = check_generate_args(1, do_sample, max_new_tokens, temperature, top_k, top_p)
        if max(self.lens) + max(len(p) for p in self.pending) + max_new_tokens - 1 > self.max_len:
            raise RuntimeError("session full: %d rows held, max_new_tokens=%d, max_len=%d" % (max(self.lens), max_new_tokens, self.max_len))
        self._push([[] for _ in self.lens])
        dev = self.logits.device
        B = len(self.lens)
        eos_ids, pad = eos_and_pad(self.config, eos_token_id, pad_token_id, dev)
        select = _argmax if sampling is None else _sampler(self.model, B, dev, *sampling, generator)
        out, real = _loop_from(self.model, self.cache, self.logits, max_new_tokens, eos_ids, pad, select, stopping_criteria, None)
        toks, real = out.tolist(), real.tolist()
        pushed = out.shape[1] - 1                       # every column but the last went through decode_step
        for b in range(B):
            held = min(real[b], pushed)
            self.lens[b] += held
            self.pending[b] = toks[b][held:real[b]]
        self._set_lens()
        return out

    @torch.no_grad()
    def fork(self, n=None, prefix_of=None, max_new=256):
        """Branch the session: -> ForkedSession whose members continue from this session's rows without copying them.  n: every row n ways
        (member b * n + i continues row b); prefix_of: the general form, a non-decreasing list of this session's row indices, one per
        member.  max_new: the own rows each member can hold (tokens generated plus ids appended).  Pending tokens are pushed first, so the
        kept logits match the cache; member m starts from logits[prefix_of[m]].  This session may go on appending and generating while its
        forks live: they read its cache only below the lengths recorded here."""
        if (n is None) == (prefix_of is None):
            raise ValueError("session.fork needs n or prefix_of (one of them)")
        if n is not None:
            if int(n) < 1:
                raise ValueError("session.fork: n=%r (needs an int >= 1)" % (n,))
            prefix_of = n_ways(len(self.lens), n)
        prefix_of = check_prefix_of(prefix_of, len(self.lens))
        if max_new is None or int(max_new) < 1:
            raise ValueError("session.fork: max_new=%r (needs an int >= 1)" % (max_new,))
        self._push([[] for _ in self.lens])
        fork = ForkCache(self.cache, prefix_of, int(max_new), self.lens)
        logits = self.logits[torch.tensor(prefix_of, dtype=torch.long, device=self.logits.device)]
        return ForkedSession(self.model, fork, logits, self.config)

    @torch.no_grad()
    def beam_search(self, num_beams, max_new_tokens, length_penalty=1.0, early_stopping=False, num_return_sequences=1, eos_token_id=None,
                    pad_token_id=None, stopping_criteria=None, do_sample=False, images=None):
        """Beam search from the session's rows, with the semantics of HF's generate(num_beams=, do_sample=False) -> BeamOutput(sequences
        [B * num_return_sequences, L] new tokens only, row b * n_ret + i best first, padded with pad; sequences_scores fp32).  Pending tokens
        are pushed first, as fork() does; the B * num_beams beams then read this session's rows in place as their prefix, up to the lengths
        recorded now, and live in a BeamCache this call allocates and drops: the session's lens, pending, logits and cache rows are left as
        after that push.  Every argument is checked before the first launch."""
        if images is not None:
            raise NotImplementedError("session.beam_search: images in a later turn are not implemented; start a new session")
        dev = self.logits.device
        eos_ids, pad = eos_and_pad(self.config, eos_token_id, pad_token_id, dev)
        V = self.logits.shape[-1]
        Kb, n_ret, C = check_beam_args(num_beams, max_new_tokens, length_penalty, early_stopping, num_return_sequences, eos_ids.numel(), V,
                                       K.beam_select_limits()[0], do_sample, stopping_criteria)
        if max(self.lens) + max(len(p) for p in self.pending) > self.max_len:
            raise RuntimeError("session full: %d rows held, %d pending, max_len=%d" % (max(self.lens), max(len(p) for p in self.pending),
                                                                                       self.max_len))
        self._push([[] for _ in self.lens])
        B = len(self.lens)
        state = BeamState(B, Kb, max_new_tokens, eos_ids.tolist(), pad, length_penalty, early_stopping, n_ret)
        beams = BeamCache(self.cache, B, Kb, max(int(max_new_tokens) - 1, 1), self.lens)
        return beam_loop(self.model, beams, self.logits, state)


# ------------------------------------------------------------------------------------------------
# forks: M members over the rows of a parent cache
def n_ways(B, n):
    """prefix_of of B rows forked n ways each: member b * n + i continues row b."""
    return [b for b in range(int(B)) for _ in range(int(n))]


def check_prefix_of(prefix_of, P):
    """-> prefix_of as a list of ints: one parent row index in [0, P) per member, non-decreasing (members of one row are contiguous)."""
    try:
        out = [int(v) for v in prefix_of]
    except TypeError:
        raise ValueError("prefix_of must be a list of ints, got %r" % (prefix_of,))
    if not out:
        raise ValueError("prefix_of is empty: a fork needs at least one member")
    if min(out) < 0 or max(out) >= P:
        raise ValueError("prefix_of holds row indices in [0, %d), got %s" % (P, out))
    if any(a > b for a, b in zip(out, out[1:])):
        raise ValueError("prefix_of must be non-decreasing (members of one prefix row are contiguous), got %s" % out)
    return out


class ForkCache:
    """M members over the rows of `parent` (a KVCache): member m reads parent row prefix_of[m] in place up to prefix_lens[prefix_of[m]] - the
    rows that row held at fork time (a host list; None = read parent.lens) - and owns k, v bf16 [M, H, Lown, D] per layer behind it, with
    own_lens int32 [layers, M] on the device.  Own row t of member m sits at position prefix_lens[prefix_of[m]] + t.  Nothing is copied
    from the parent, and its slots at or beyond the recorded lengths are never read: it may go on appending while forks live."""

    def __init__(self, parent, prefix_of, Lown, prefix_lens=None):
        prefix_of = check_prefix_of(prefix_of, parent.B)
        if int(Lown) < 1:
            raise ValueError("a fork needs Lown >= 1 own slots, got %r" % (Lown,))
        lens = parent.lens[0].tolist() if prefix_lens is None else [int(v) for v in prefix_lens]
        if len(lens) != parent.B:
            raise ValueError("prefix_lens needs one length per parent row (%d), got %d" % (parent.B, len(lens)))
        used = sorted(set(prefix_of))
        if any(lens[p] < 1 or lens[p] > parent.Lcap for p in used):
            raise ValueError("every forked row needs between 1 and %d rows in the parent, got %s" % (parent.Lcap, [lens[p] for p in used]))
        dev = parent.k[0].device
        n = len(parent.k)
        M, H, D = len(prefix_of), parent.H, parent.D
        self.parent, self.M, self.P, self.H, self.D, self.Lown = parent, M, parent.B, H, D, int(Lown)
        self.host_prefix_of, self.host_prefix_lens = prefix_of, lens
        self.prefix_of = torch.tensor(prefix_of, dtype=torch.int32, device=dev)
        self.prefix_lens = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.k = [torch.empty(M, H, self.Lown, D, dtype=torch.bfloat16, device=dev) for _ in range(n)]
        self.v = [torch.empty(M, H, self.Lown, D, dtype=torch.bfloat16, device=dev) for _ in range(n)]
        self.own_lens = torch.zeros(n, M, dtype=torch.int32, device=dev)
        self.filled = 0            # host-side upper bound of max_m own_lens[m], as KVCache.filled
        self.ws = torch.empty(max(K.fork_ws_bytes(M, H, parent.Lcap, self.Lown), 16), dtype=torch.uint8, device=dev)
        need = max(lens[p] for p in used) + self.Lown
        cos, sin = parent.cos, parent.sin
        if cos.shape[0] < need:
            cos, sin = parent.rope(need, dev)
        if cos.shape[0] < need:
            # the append kernels skip a row whose position lies beyond the tables, and the attention would then run without it
            raise RuntimeError("RoPE tables of %d rows do not cover the fork's %d positions" % (cos.shape[0], need))
        self.cos, self.sin = cos, sin

    # the surface shared with KVCache (see the module docstring); lens and Lcap are what DecodeSession and the messages read
    full_step = "KV cache full: %d own slots used of %d; fork with max_new for every new token"
    rows_refusal = None
    lens = property(lambda self: self.own_lens)
    Lcap = property(lambda self: self.Lown)
    rows = property(lambda self: self.M)
    room = property(lambda self: self.Lown)

    def attend_step(self, layer_idx, qkv, H, D, out_width):
        """The new row is appended to the member's own rows and attends the parent's prefix row, read in place, followed by the own rows."""
        K.fork_rope_append(qkv, self.cos, self.sin, self.prefix_lens, self.prefix_of, self.k[layer_idx], self.v[layer_idx],
                           self.own_lens[layer_idx], H, D)
        return self._step_attention(qkv, self.parent.k[layer_idx], self.parent.v[layer_idx], self.k[layer_idx], self.v[layer_idx],
                                    self.own_lens[layer_idx], H, D, out_width)

    def _step_attention(self, qkv, pk, pv, kc, vc, lens, H, D, out_width):
        return K.fork_decode_attention(qkv, pk, pv, self.prefix_lens, self.prefix_of, kc, vc, lens, self.ws, H, D, out_width)

    def attend_rows(self, layer_idx, qkv, n_new_d, H, D, out_width):
        pk, pv = self.parent.k[layer_idx], self.parent.v[layer_idx]
        kc, vc, lens = self.k[layer_idx], self.v[layer_idx], self.own_lens[layer_idx]
        K.fork_extend_rope_append(qkv, self.cos, self.sin, self.prefix_lens, self.prefix_of, kc, vc, lens, n_new_d, H, D)
        a = K.fork_extend_attention(qkv, pk, pv, self.prefix_lens, self.prefix_of, kc, vc, lens, n_new_d, H, D, out_width)
        K.extend_advance(lens, n_new_d, self.Lown)
        return a


class BeamCache(ForkCache):
    """The ForkCache of beam search: B prompts x K beams, member b * K + i reads parent row b.  anc int32 [2, M, Lown] on the device is one
    double-buffered ancestry table for all layers, `cur` the half in use: anc[cur][m][t], t < own rows, is the member whose own slot t holds
    row t of member m's history.  All members advance in lockstep (a prompt that is done steps on pad), so every own_lens[l][m] is the same
    number, `filled` on the host.  K / V rows are never copied or moved."""

    def __init__(self, parent, B, num_beams, Lown, prefix_lens=None):
        if int(B) != parent.B:
            raise ValueError("a BeamCache needs one group of beams per parent row (%d), got B=%r" % (parent.B, B))
        if int(num_beams) < 1:
            raise ValueError("a BeamCache needs num_beams >= 1, got %r" % (num_beams,))
        super().__init__(parent, n_ways(B, num_beams), Lown, prefix_lens)
        self.B, self.num_beams = int(B), int(num_beams)
        self.anc = torch.zeros(2, self.M, self.Lown, dtype=torch.int32, device=self.k[0].device)
        self.cur = 0

    full_step = "KV cache full: %d own slots used of %d; allocate the BeamCache for every pushed token"
    rows_refusal = ("a BeamCache takes one row per member and step (beam_decode_step): pushing several rows through the ancestry table is "
                    "not implemented")

    @property
    def table(self):
        return self.anc[self.cur]

    def _step_attention(self, qkv, pk, pv, kc, vc, lens, H, D, out_width):
        """The own rows are read through the ancestry table (whose slot holds row t of the member's history)."""
        return K.beam_decode_attention(qkv, pk, pv, self.prefix_lens, self.prefix_of, kc, vc, lens, self.table, self.ws, H, D, out_width)

    def attend_rows(self, layer_idx, qkv, n_new_d, H, D, out_width):
        raise NotImplementedError(self.rows_refusal)


@torch.no_grad()
def beam_decode_step(model, beams, token_ids, parents):
    """One step of every beam: member m pushes token_ids[m] behind the history of member parents[m] (int32 [M] on the device) -> logits
    [M, V] fp32.  One halva_beam_advance writes the other half of the ancestry table from the current one and the parents, the halves swap,
    and decode_step runs: each layer appends its k / v at own slot own_lens[m] of member m and attends through the table."""
    _check_room(beams)          # before the table moves: a refused step leaves cur, filled and both halves as they were
    nxt = 1 - beams.cur
    K.beam_advance(beams.anc[beams.cur], beams.anc[nxt], parents.to(beams.anc.device, torch.int32), beams.own_lens[0])
    beams.cur = nxt
    return decode_step(model, beams, token_ids)


@torch.no_grad()
def beam_loop(model, beams, logits, state, step=None):
    """The beam loop from (a BeamCache over the prompts' rows, their last-row logits [B, V] fp32, a fresh BeamState) -> BeamOutput.  Per step:
    one halva_beam_select launch pair on the M rows, ONE host sync that brings its three [B, C] tensors over, BeamState.step on the host,
    beam_decode_step.  A live prompt whose rows leave nothing to select (NaN or inf logits, or none above -inf) raises RuntimeError on that
    sync.  step: the function that pushes a column (None = beam_decode_step; tests pass a materialising twin)."""
    B, Kb, C = state.B, state.K, state.C
    dev = logits.device
    logits = logits[torch.arange(B, device=dev).repeat_interleave(Kb)]
    while True:
        score, token, beam = K.beam_select(logits, state.run_scores.view(-1).to(dev), Kb, C)
        host = torch.cat([score.view(torch.int32).view(-1), token.view(-1), beam.view(-1)]).cpu()          # the step's one host sync
        score, token, beam = host[:B * C].view(torch.float32).view(B, C), host[B * C:2 * B * C].view(B, C), host[2 * B * C:].view(B, C)
        bad = (token < 0).any(1) & ~state.closed()
        if bool(bad.any()):
            raise RuntimeError("beam_search: prompt %d has no token to select at step %d (NaN or inf logits, or none above -inf)"
                               % (int(bad.nonzero()[0]), state.n))
        nxt, parents, finished = state.step(score, token, beam)
        if finished:
            break
        logits = (step or beam_decode_step)(model, beams, nxt.to(dev), parents.to(dev, torch.int32))
    out = state.finalize()
    return BeamOutput(out.sequences.to(dev), out.sequences_scores.to(dev))


@torch.no_grad()
def sample_fork(model, inputs_embeds, seq_len, n, max_new_tokens, eos_ids, pad, temperature, top_k, top_p, generator=None,
                stopping_criteria=None, prefix=None, prefill_chunk=None):
    """sample() with n continuations per prompt (generate's num_return_sequences): ONE prompt pass at batch B into a cache of the prompt's
    rows, a fork n ways, and the sampled loop on the B * n members (member b * n + i continues prompt b) -> LongTensor [B * n, len].  Each
    step draws u = torch.rand(B * n, generator=generator) exactly once, done members included."""
    B, T = inputs_embeds.shape[0], inputs_embeds.shape[1]
    select = _sampler(model, B * n, inputs_embeds.device, temperature, top_k, top_p, generator)
    cache = KVCache(model, B, T, inputs_embeds.device)
    logits = prompt_pass(model, inputs_embeds, seq_len, cache, prefill_chunk)
    prefix_of = n_ways(B, n)
    fork = ForkCache(cache, prefix_of, max_new_tokens, [int(v) for v in seq_len])
    logits = logits[torch.tensor(prefix_of, dtype=torch.long, device=logits.device)]
    return _loop_from(model, fork, logits, max_new_tokens, eos_ids, pad, select, stopping_criteria, prefix)[0]


class ForkedSession(DecodeSession):
    """The members of DecodeSession.fork(): generate() and append() with DecodeSession's signatures and rules, on a ForkCache.  lens[m] counts
    the member's OWN rows (max_len = the fork's max_new); member m's history is row prefix_of[m] of the parent up to prefix_lens[m] and
    then its own rows."""

    def __init__(self, model, fork, logits, config=None):
        super().__init__(model, fork, logits, [0] * fork.M, config)
        self.prefix_of = list(fork.host_prefix_of)
        self.prefix_lens = [fork.host_prefix_lens[p] for p in self.prefix_of]

    def fork(self, n=None, prefix_of=None, max_new=256):
        raise NotImplementedError("forks of forks are not implemented; fork the parent session again")

    def beam_search(self, *args, **kwargs):
        raise NotImplementedError("beam search from a forked session is not implemented; call beam_search on the parent session")
