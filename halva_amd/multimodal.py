"""What the LLaVA wrapper (halva_amd/llava_model.py) and the VILA wrapper (halva_amd/vila_model.py) share: the splice
contract, the decoder pass over spliced embeddings, the logits / CE tail of `forward`, greedy generation and the
description the step engine (halva_amd/dpa.py) asks for - each written once, in `MultimodalMixin`.

A wrapper supplies what really differs:
  get_model()              the Llama stack (embed_tokens / layers / run_layers)
  lm_head                  the output projection
  get_vision_tower()       the frozen tower, or None
  _lm_config()             the config that carries tokenizer_model_max_length / tokenizer_padding_side / eos / pad ids
  _image_features(...)     images -> (features [n, tokens, d], image_map or None)
  _tokens_per_image()      image tokens per image after the projector
  causal_lm(), projector() (module, parameter-name prefix) pairs for the flat trainable buffer
and the four class attributes below.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import kernels as K
from . import splice as SP

IGNORE_INDEX = -100
IMAGE_TOKEN_INDEX = -200
_LEFT_PADDED = "%s: left-padded prompts are not supported; pad on the right and pass attention_mask"


class CausalLMOutput(SimpleNamespace):
    pass


def _cpu(t):
    return t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(t)


class BaseOnlyLayer(nn.Module):
    """A decoder layer that reuses another layer's frozen base tensors and never applies its LoRA factors."""

    def __init__(self, layer):
        super().__init__()
        self._l = [layer]            # not registered: the tensors belong to the policy model

    def forward(self, x, info, use_lora=False, own_x=False, rows=None):
        return self._l[0](x, info, False, own_x, rows)


class FrozenProjectorView(nn.Module):
    """Another model's projector, run under no_grad; `kind`, `config` and `tokens_per_image` (VILA's MultimodalProjector) are
    forwarded when the projector has them."""

    def __init__(self, proj):
        super().__init__()
        self._p = [proj]             # not registered, see BaseOnlyLayer
        for a in ("kind", "config", "tokens_per_image"):
            if hasattr(proj, a):
                setattr(self, a, getattr(proj, a))

    def forward(self, x, *a, **k):
        with torch.no_grad():
            return self._p[0](x)


def reuse_base(llama, src_llama):
    """The reference model == base of the policy: `llama` (built with no layers) takes the policy's frozen tensors."""
    llama.embed_tokens = src_llama.embed_tokens
    llama.norm = src_llama.norm
    llama.layers = nn.ModuleList([BaseOnlyLayer(l) for l in src_llama.layers])


def random_fill_(named_params, g, std, is_norm=lambda n: "ln" in n or "norm" in n):
    """Weights N(0, std) from generator `g` in iteration order, norm weights 1 and norm biases 0 (no draw)."""
    for n, p in named_params:
        if p.ndim < 2 and is_norm(n):
            p.zero_() if (n.endswith("_b") or n.endswith("bias")) else p.fill_(1.0)
        else:
            p.normal_(0.0, std, generator=g)


class MultimodalMixin:
    imageless_consumes = True        # an image-less row still advances the running image index (LLaVA; VILA: False)
    ce_none_without_targets = False  # forward()'s CE on all-ignored labels: mean of an empty tensor (LLaVA) or None (VILA)
    left_padding_refused_before_splice = False      # generate(): VILA checks the given mask, LLaVA the spans after the splice
    generate_returns_prompt = True   # generate() -> [prompt | new] (LLaVA) or the new tokens only (VILA)

    @property
    def device(self):
        return self.lm_head.weight.device

    @property
    def dtype(self):
        return self.lm_head.weight.dtype

    # -- what the step engine needs (halva_amd/dpa.py) -------------------------------------------
    def dpa_spec(self):
        """Image tokens per image after the projector, the post-splice truncation length and padding side, and whether an
        image-less row advances the image index."""
        lc = self._lm_config()
        return SimpleNamespace(n_patch=self._tokens_per_image(), max_len=getattr(lc, "tokenizer_model_max_length", None),
                               padding_side=getattr(lc, "tokenizer_padding_side", "right"),
                               imageless_consumes=self.imageless_consumes)

    def hidden_states(self, inputs_embeds, attention_mask=None, seq_start=None, seq_len=None, branch=None, rows=None):
        """Decoder stack + final norm on inputs_embeds [S, T, d].  The key-padding mask must be one contiguous run per
        row (what the splice produces); it is the raw [S, T] bool mask of the flash-attn seam
        (llama_flash_attn_monkey_patch.py:71,98-102)."""
        S, T, _ = inputs_embeds.shape
        dev = inputs_embeds.device
        if seq_len is None:
            if attention_mask is None:
                seq_start = torch.zeros(S, dtype=torch.int32)
                seq_len = torch.full((S,), T, dtype=torch.int32)
            elif self._last_plan is not None and self._last_plan.mask.shape == attention_mask.shape:
                seq_start, seq_len = self._last_plan.seq_start, self._last_plan.seq_len     # no device sync
            else:
                seq_start, seq_len = SP.spans_from_mask(_cpu(attention_mask))
        return self.get_model().run_layers(inputs_embeds.to(torch.bfloat16), seq_start.to(dev), seq_len.to(dev), self._use_lora,
                                           branch, rows)

    # -- the splice ------------------------------------------------------------------------------
    def _splice(self, input_ids, attention_mask, labels, signs, images, **given):
        """Index plan on the host + one gather launch (halva_amd/splice.py); the plan is kept as `_last_plan`."""
        feats, image_map = self._image_features(input_ids, attention_mask, images, **given)
        lc = self._lm_config()
        plan = SP.plan_splice(_cpu(input_ids), None if attention_mask is None else _cpu(attention_mask),
                              None if labels is None else _cpu(labels), None if signs is None else _cpu(signs),
                              n_patch=feats.shape[1], max_len=getattr(lc, "tokenizer_model_max_length", None),
                              padding_side=getattr(lc, "tokenizer_padding_side", "right"), image_map=image_map,
                              imageless_consumes=self.imageless_consumes)
        embeds = K.splice_rows(self.get_model().embed_tokens.weight, feats.to(torch.bfloat16), plan.src, plan.S, plan.T)
        self._last_plan = plan
        return embeds, plan

    def prepare_inputs_labels_for_multimodal_signed(self, input_ids, position_ids, attention_mask, past_key_values, labels,
                                                    images, signs):
        if self.get_vision_tower() is None or images is None or input_ids.shape[1] == 1:
            return input_ids, position_ids, attention_mask, past_key_values, None, labels, signs
        embeds, plan = self._splice(input_ids, attention_mask, labels, signs, images)
        dev = input_ids.device
        new_mask = None if attention_mask is None else plan.mask.to(dev).to(attention_mask.dtype)
        return (None, position_ids, new_mask, past_key_values, embeds, None if labels is None else plan.labels.to(dev),
                None if signs is None else plan.signs.to(dev))

    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images):
        return self.prepare_inputs_labels_for_multimodal_signed(input_ids, position_ids, attention_mask, past_key_values, labels,
                                                                images, None)[:6]

    # -- forward ---------------------------------------------------------------------------------
    def _forward_multimodal(self, input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, labels, use_cache,
                            images, signs=None):
        """The body of `forward`: splice (unless inputs_embeds is given), decoder pass, full fp32 logits and the CE on the kept
        targets.  Returns (output, labels, signs) with the post-splice labels / signs."""
        if past_key_values is not None or use_cache:
            raise NotImplementedError("KV-cache decoding is not part of the DPA training path")
        if inputs_embeds is None:
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels,
             signs) = self.prepare_inputs_labels_for_multimodal_signed(input_ids, position_ids, attention_mask, past_key_values,
                                                                       labels, images, signs)
            if inputs_embeds is None:
                inputs_embeds = self.get_model().embed_tokens(input_ids)
        h = self.hidden_states(inputs_embeds, attention_mask)
        logits = torch.nn.functional.linear(h, self.lm_head.weight).float()
        loss = None
        if labels is not None:
            tgt = labels[..., 1:].contiguous().view(-1)
            keep = (tgt != IGNORE_INDEX).nonzero().flatten()
            if keep.numel() or not self.ce_none_without_targets:
                lg = logits[..., :-1, :].reshape(-1, logits.shape[-1])
                loss = -K.token_logp(lg[keep].contiguous(), tgt[keep].int()).mean()
        out = CausalLMOutput(loss=loss, logits=logits, past_key_values=None, hidden_states=None, attentions=None)
        return out, labels, signs

    # -- inference / export ----------------------------------------------------------------------
    def merge_and_unload(self):
        """peft's merge_and_unload, as the reference's loaders call it before evaluation: every LoRA group of the Llama stack is
        folded into its base weight (halva_amd/llama.py:LlamaModel.merge_and_unload) and the model runs LoRA-free from then on.
        A second call is a no-op; a model a trainer has bound (gradient sink set) is refused.  Returns self."""
        self.get_model().merge_and_unload()
        self._use_lora = False
        return self

    # -- generation ------------------------------------------------------------------------------
    def decode_stack(self):
        """The pieces the KV-cached decode runs on (halva_amd/decode.py): the Llama stack and the head."""
        from .decode import DecodeStack
        return DecodeStack(self.get_model(), self.lm_head.weight, self._use_lora)

    def _embed_prompt(self, input_ids, images, attention_mask, who="generate"):
        """The front part of generation: the prompt spliced when there are images, a tower and more than one token, else embedded.
        Right padding only.  -> (inputs_embeds [B, T, d], seq_len int32 [B] on the host)."""
        if input_ids is None or input_ids.ndim != 2:
            raise ValueError("%s needs input_ids [B, T]" % who)
        dev = self.device
        ids = input_ids.to(dev)
        mask = None if attention_mask is None else attention_mask.to(dev)
        B, T0 = ids.shape
        if self.left_padding_refused_before_splice and mask is not None and int(SP.spans_from_mask(_cpu(mask))[0].max()) != 0:
            raise NotImplementedError(_LEFT_PADDED % who)      # (the splice would re-pad such rows to the right)
        embeds = None
        if images is not None:
            images = [im.to(dev, torch.bfloat16) for im in images] if type(images) is list else images.to(dev, torch.bfloat16)
            self._last_plan = None
            _, _, _, _, embeds, _ = self.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, images)
        if embeds is not None:
            seq_start, seq_len = self._last_plan.seq_start, self._last_plan.seq_len
        else:
            if (ids < 0).any():
                raise ValueError("input_ids hold image tokens but no images (or no vision tower) were given")
            embeds = self.get_model().embed_tokens(ids)
            if mask is None:
                seq_start, seq_len = torch.zeros(B, dtype=torch.int32), torch.full((B,), T0, dtype=torch.int32)
            else:
                seq_start, seq_len = SP.spans_from_mask(_cpu(mask))
        if int(seq_start.max()) != 0:
            raise NotImplementedError(_LEFT_PADDED % who)
        return embeds, seq_len

    @torch.no_grad()
    def _generate(self, input_ids, images, attention_mask, do_sample, num_beams, max_new_tokens, eos_token_id, pad_token_id,
                  stopping_criteria, temperature=None, top_k=None, top_p=None, generator=None, prefill_chunk=None, num_return_sequences=1,
                  images_cd=None, negative_input_ids=None, negative_attention_mask=None, cd_alpha=None, cd_beta=None, guidance_scale=None):
        """The body of `generate`: _embed_prompt, then halva_amd/decode.py:greedy, or :sample when do_sample is set.  prefill_chunk: None =
        one prompt pass; an int >= 1 = the prompt pass in blocks of that many rows (decode.prefill_chunked).  num_return_sequences = n > 1
        (sampling only, as in HF): one prompt pass, then n continuations per prompt over a forked cache (decode.sample_fork) -> rows
        b * n + i, with the prompt repeated where the prompt is returned.  images_cd (the same ids over other images) or negative_input_ids
        / negative_attention_mask (another prompt; its image tokens, if any, take `images`) turn on contrastive decoding
        (decode.contrast) with cd_alpha (None = 0.5) and cd_beta (None = 0.1), or guidance_scale = 1 + alpha with beta = 0; without them the
        call runs exactly as before."""
        from . import decode as DEC
        cd = DEC.check_contrast_args(images_cd is not None, negative_input_ids is not None, negative_attention_mask is not None, cd_alpha,
                                     cd_beta, guidance_scale, num_beams, num_return_sequences)
        sampling = DEC.check_generate_args(num_beams, do_sample, max_new_tokens, temperature, top_k, top_p)
        n_ret = 1 if num_return_sequences is None else int(num_return_sequences)
        if n_ret < 1:
            raise ValueError("generate: num_return_sequences=%r (needs an int >= 1)" % (num_return_sequences,))
        if n_ret > 1 and sampling is None:
            raise ValueError("generate: num_return_sequences=%d needs do_sample=True: greedy decoding returns one sequence per prompt" % n_ret)
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("generate: prefill_chunk=%r (needs an int >= 1, or None)" % (prefill_chunk,))
        embeds, seq_len = self._embed_prompt(input_ids, images, attention_mask)
        dev = self.device
        eos_ids, pad = DEC.eos_and_pad(self._lm_config(), eos_token_id, pad_token_id, dev)
        prompt = input_ids.to(dev) if self.generate_returns_prompt else None
        if cd is not None:
            if images_cd is not None:
                embeds_cd, seq_len_cd = self._embed_prompt(input_ids, images_cd, attention_mask)
            else:
                if negative_input_ids.ndim != 2 or negative_input_ids.shape[0] != input_ids.shape[0]:
                    raise ValueError("generate: negative_input_ids needs one row per prompt [B=%d, T']" % input_ids.shape[0])
                embeds_cd, seq_len_cd = self._embed_prompt(negative_input_ids, images if bool((negative_input_ids < 0).any()) else None,
                                                           negative_attention_mask)
            out = DEC.contrast(self, embeds, seq_len, embeds_cd, seq_len_cd, max_new_tokens, eos_ids, pad, *cd, sampling=sampling,
                               generator=generator, stopping_criteria=stopping_criteria, prefix=prompt, prefill_chunk=prefill_chunk)
        elif n_ret > 1:
            prompt = None if prompt is None else prompt.repeat_interleave(n_ret, 0)
            out = DEC.sample_fork(self, embeds, seq_len, n_ret, max_new_tokens, eos_ids, pad, *sampling, generator=generator,
                                  stopping_criteria=stopping_criteria, prefix=prompt, prefill_chunk=prefill_chunk)
        elif sampling is None:
            out = DEC.greedy(self, embeds, seq_len, max_new_tokens, eos_ids, pad, stopping_criteria, prefix=prompt, prefill_chunk=prefill_chunk)
        else:
            out = DEC.sample(self, embeds, seq_len, max_new_tokens, eos_ids, pad, *sampling, generator=generator,
                             stopping_criteria=stopping_criteria, prefix=prompt, prefill_chunk=prefill_chunk)
        return out if prompt is None else torch.cat([prompt.long(), out], 1)

    def _prompt_session(self, embeds, seq_len, max_len, prefill_chunk):
        """A cache of max_len slots and the prompt pass over an embedded prompt (_embed_prompt's pair), in blocks of prefill_chunk rows when
        given -> decode.DecodeSession on that cache with the last-row logits kept."""
        from . import decode as DEC
        cache = DEC.KVCache(self, embeds.shape[0], int(max_len), embeds.device)
        logits = DEC.prompt_pass(self, embeds, seq_len, cache, prefill_chunk)
        cache.filled = int(seq_len.max())
        return DEC.DecodeSession(self, cache, logits, seq_len.tolist(), self._lm_config())

    @torch.no_grad()
    def beam_search(self, input_ids, images=None, attention_mask=None, num_beams=1, max_new_tokens=None, length_penalty=1.0,
                    early_stopping=False, num_return_sequences=1, eos_token_id=None, pad_token_id=None, stopping_criteria=None, do_sample=False,
                    prefill_chunk=None):
        """Beam search with the semantics of HF's generate(num_beams=, do_sample=False) -> decode.BeamOutput(sequences [B * n_ret, L],
        sequences_scores [B * n_ret]): the new tokens only, on both model families.  _embed_prompt, ONE prompt pass at batch B into a cache of
        the prompt's rows, then DecodeSession.beam_search on it: the B * num_beams beams read those rows in place and no K / V row moves when
        a beam continues another beam (decode.BeamCache).  Every argument rule is checked before the first launch.  generate(num_beams > 1)
        still raises NotImplementedError."""
        from . import decode as DEC
        from . import kernels as K
        from .beam import check_beam_args
        eos_ids, _ = DEC.eos_and_pad(self._lm_config(), eos_token_id, pad_token_id, "cpu")
        check_beam_args(num_beams, max_new_tokens, length_penalty, early_stopping, num_return_sequences, eos_ids.numel(),
                        self.lm_head.weight.shape[0], K.beam_select_limits()[0], do_sample, stopping_criteria)
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("beam_search: prefill_chunk=%r (needs an int >= 1, or None)" % (prefill_chunk,))
        embeds, seq_len = self._embed_prompt(input_ids, images, attention_mask, "beam_search")
        session = self._prompt_session(embeds, seq_len, embeds.shape[1], prefill_chunk)
        return session.beam_search(num_beams, max_new_tokens, length_penalty, early_stopping, num_return_sequences, eos_token_id, pad_token_id)

    @torch.no_grad()
    def start_session(self, input_ids, images=None, attention_mask=None, max_len=None, prefill_chunk=None):
        """A decoding session that keeps its KV cache between calls (halva_amd/decode.py:DecodeSession): the prompt is spliced and embedded
        exactly as generate() does, a cache of max_len slots (default: tokenizer_model_max_length, else the prompt's rows + 256) is
        allocated and prefilled (in blocks of prefill_chunk rows when given), and the last-row logits are kept.  Then
        session.generate(max_new_tokens, ...) -> the new tokens [B, n], session.append(input_ids, attention_mask) for a text-only next
        turn; session.lens is the host list of rows held per sequence."""
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("start_session: prefill_chunk=%r (needs an int >= 1, or None)" % (prefill_chunk,))
        embeds, seq_len = self._embed_prompt(input_ids, images, attention_mask)
        T = embeds.shape[1]
        if max_len is None:
            max_len = max(getattr(self._lm_config(), "tokenizer_model_max_length", None) or 0, T + 256)
        if int(max_len) < T:
            raise ValueError("start_session: max_len=%d is below the prompt's %d rows" % (max_len, T))
        return self._prompt_session(embeds, seq_len, max_len, prefill_chunk)
