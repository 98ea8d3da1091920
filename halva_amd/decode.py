"""KV-cached greedy decoding for LLaVA-1.5 (LlavaLlamaForCausalLM.generate) - forward only.

Stands in for the reference's HF `generate(..., use_cache=True)` decode path: the per-layer cache concat
(llava/model/language_model/modelling_llama.py:295-305) and the decode position rule `attention_mask.sum(1) - 1`
(llava/model/llava_arch.py:90-98) become halva_decode_rope_append, the single-query attention halva_decode_attn
(split-KV; include/halva_hip.h).  Everything else of a decode step is the training path's own pieces on [B, d] rows.

Cache layout, per layer: K, V bf16 [B, H, Lcap, D]; lens int32 [layers, B] on the device (each layer's append advances its own
row).  Prompts are right-padded: sequence b holds positions [0, seq_len[b]).
"""
import torch

from . import kernels as K


class KVCache:
    """[layers][K, V] bf16 [B, H, Lcap, D], lens int32 [layers, B] and the split-KV workspace, allocated once per generate call."""

    def __init__(self, model, B, Lcap, device=None):
        cfg = model.config
        lm = model.get_model()
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


def _lm_head(model, h):
    return torch.nn.functional.linear(h, model.lm_head.weight).float()


@torch.no_grad()
def prefill(model, inputs_embeds, seq_len, cache):
    """The prompt pass: run_layers on right-padded inputs_embeds [B, T, d] (sequence b = rows [0, seq_len[b])) with the cache fill
    hooked into every layer; the top layer runs only the last prompt row of each sequence.  -> last-row logits [B, V] fp32."""
    lm = model.get_model()
    B, T, _ = inputs_embeds.shape
    dev = inputs_embeds.device
    seq_len = torch.as_tensor(seq_len, dtype=torch.int32)
    if int(seq_len.min()) < 1 or int(seq_len.max()) > T:
        raise ValueError("every prompt needs between 1 and T=%d rows" % T)
    seq_len_d = seq_len.to(dev)
    rows = (torch.arange(B, dtype=torch.int64) * T + seq_len.long() - 1).to(dev)
    h = lm.run_layers(inputs_embeds.to(torch.bfloat16), torch.zeros(B, dtype=torch.int32, device=dev), seq_len_d, model._use_lora, None, rows,
                      kv_hook=lambda i, qkv: cache.fill(i, qkv, seq_len_d))
    return _lm_head(model, h)


@torch.no_grad()
def decode_step(model, cache, token_ids):
    """One new token per sequence: token_ids [B] -> logits [B, V] fp32.  Appends each layer's k / v at slot lens[b]."""
    if cache.filled >= min(cache.Lcap, cache.cos.shape[0]):
        # the append kernel leaves a full cache untouched (it never writes out of bounds): refuse here instead of attending without
        # the new token
        raise RuntimeError("KV cache full: %d slots used of %d; allocate the cache for the prompt plus every new token" % (cache.filled, cache.Lcap))
    cache.filled += 1
    lm = model.get_model()
    x = lm.embed_tokens(token_ids.to(lm.embed_tokens.weight.device).long())          # a fresh buffer: the residual adds run on it in place
    for i, layer in enumerate(lm.layers):
        x = layer.decode(x, cache, i, model._use_lora)
    return _lm_head(model, lm.norm(x))
