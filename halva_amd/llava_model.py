"""LlavaLlamaForCausalLM for the DPA step (MI355X-native), keeping the reference's API surface:

reference llava/model/language_model/llava_llama.py:16-97 (LlavaConfig, LlavaLlamaModel, LlavaLlamaForCausalLM)
reference llava/model/llava_arch.py:13-440 (LlavaMetaModel, LlavaMetaForCausalLM: encode_images,
prepare_inputs_labels_for_multimodal[_signed], initialize_vision_modules / _tokenizer).

The splice is a host-computed index plan + one gather launch (halva_amd/splice.py); logits for the loss are
normally never materialised (halva_amd/dpa.py fuses lm_head with the loss kernels), `forward()` still returns
full fp32 logits for API parity with `LlamaForCausalLM.forward(...).logits.float()` (modelling_llama.py:806).
"""
import os

import torch
import torch.nn as nn

from .clip import CLIPVisionTower, _read_checkpoint, build_vision_projector, build_vision_tower
from .llama import (LlamaConfig, LlamaModel, add_lora, hf_llama_state_dict, load_hf_llama_weights)
from .multimodal import (IGNORE_INDEX, IMAGE_TOKEN_INDEX, CausalLMOutput, FrozenProjectorView, MultimodalMixin,  # noqa: F401
                         _cpu, random_fill_, reuse_base)


class LlavaConfig(LlamaConfig):
    model_type = "llava"


class LlavaMetaModel:
    """reference llava/model/llava_arch.py:13-68"""

    def get_vision_tower(self):
        vt = getattr(self, "vision_tower", None)
        if type(vt) is list:
            vt = vt[0]
        return vt

    def initialize_vision_modules(self, model_args, fsdp=None):
        vision_tower = model_args.vision_tower
        self.config.mm_vision_tower = vision_tower
        if self.get_vision_tower() is None:
            vt = build_vision_tower(model_args, dtype=self._dtype, device=self._device)
            self.vision_tower = [vt] if fsdp else vt
        else:
            vt = self.get_vision_tower()
            vt.load_model()
        self.config.use_mm_proj = True
        self.config.mm_projector_type = getattr(model_args, "mm_projector_type", "linear")
        self.config.mm_hidden_size = vt.hidden_size
        self.config.mm_vision_select_layer = model_args.mm_vision_select_layer
        self.config.mm_vision_select_feature = getattr(model_args, "mm_vision_select_feature", "patch")
        if getattr(self, "mm_projector", None) is None:
            self.mm_projector = build_vision_projector(self.config, dtype=self._dtype, device=self._device)
        else:
            for p in self.mm_projector.parameters():          # "In case it is frozen by LoRA" (llava_arch.py:58-61)
                p.requires_grad = True
        ckpt = getattr(model_args, "pretrain_mm_mlp_adapter", None)
        if ckpt is not None:
            w = torch.load(ckpt, map_location="cpu")
            self.mm_projector.load_state_dict({k.split("mm_projector.")[1]: v for k, v in w.items() if "mm_projector" in k})


class LlavaLlamaModel(LlavaMetaModel, LlamaModel):
    config_class = LlavaConfig

    def __init__(self, config, dtype=torch.bfloat16, device="cuda"):
        LlamaModel.__init__(self, config, dtype, device)
        self._dtype, self._device = dtype, device
        if hasattr(config, "mm_vision_tower"):
            self.vision_tower = build_vision_tower(config, delay_load=True, dtype=dtype, device=device)
            self.mm_projector = build_vision_projector(config, dtype=dtype, device=device)


class LlavaMetaForCausalLM(MultimodalMixin):
    """reference llava/model/llava_arch.py:71-440; the splice, forward tail and generation are halva_amd/multimodal.py's."""

    def get_vision_tower(self):
        return self.get_model().get_vision_tower()

    def encode_images(self, images):
        feats = self.get_model().get_vision_tower()(images)
        return self.get_model().mm_projector(feats)

    def _image_features(self, input_ids, attention_mask, images, image_features=None, image_map=None):
        """Precomputed image_features / image_map are taken as given; a list or 5-D input is concatenated: multi-image samples
        consume the features in order, one [n_patch, d] block per image token."""
        if image_features is None:
            if type(images) is list or images.ndim == 5:
                images = torch.cat([im for im in images], dim=0)
            image_features = self.encode_images(images)
        return image_features, image_map

    def resize_token_embeddings(self, new_num_tokens):
        """HF PreTrainedModel.resize_token_embeddings for this model's two vocabulary-sized tensors: old rows kept, new rows
        N(0, initializer_range) as HF initialises them (the callers below overwrite them with the mean of the old rows)."""
        emb, head = self.get_input_embeddings(), self.get_output_embeddings()
        old = emb.weight.shape[0]
        if new_num_tokens == old:
            return emb
        std = getattr(self.config, "initializer_range", 0.02)
        for mod in (emb, head):
            w = mod.weight.data
            nw = torch.empty(new_num_tokens, w.shape[1], dtype=w.dtype, device=w.device).normal_(0.0, std)
            n = min(old, new_num_tokens)
            nw[:n] = w[:n]
            mod.weight = nn.Parameter(nw, requires_grad=mod.weight.requires_grad)
        if hasattr(emb, "num_embeddings"):
            emb.num_embeddings = new_num_tokens
        if hasattr(head, "out_features"):
            head.out_features = new_num_tokens
        self.config.vocab_size = new_num_tokens
        return emb

    def initialize_vision_tokenizer(self, model_args, tokenizer):
        """reference llava/model/llava_arch.py:398-440: <im_patch> / <im_start>, <im_end> tokens appended to the vocabulary, the new
        rows of embed_tokens and lm_head set to the mean of the old ones (or taken from --pretrain_mm_mlp_adapter).  The HALVA
        scripts pass both flags False (src/hallava_7b.sh:42-43), in which case this is a no-op, as in the reference.  Training the
        embedding matrix itself (tune_mm_mlp_adapter + mm_use_im_start_end) is not on the DPA path and is refused."""
        from llava.constants import DEFAULT_IMAGE_PATCH_TOKEN, DEFAULT_IM_END_TOKEN, DEFAULT_IM_START_TOKEN
        if getattr(model_args, "mm_use_im_patch_token", False):
            tokenizer.add_tokens([DEFAULT_IMAGE_PATCH_TOKEN], special_tokens=True)
            self.resize_token_embeddings(len(tokenizer))
        if getattr(model_args, "mm_use_im_start_end", False):
            if getattr(model_args, "tune_mm_mlp_adapter", False):
                raise NotImplementedError("tune_mm_mlp_adapter with mm_use_im_start_end trains embed_tokens (llava_arch.py:419-423): "
                                          "the MI355X DPA engine keeps the embedding matrix frozen")
            num_new = tokenizer.add_tokens([DEFAULT_IM_START_TOKEN, DEFAULT_IM_END_TOKEN], special_tokens=True)
            self.resize_token_embeddings(len(tokenizer))
            if num_new > 0:
                with torch.no_grad():
                    for w in (self.get_input_embeddings().weight, self.get_output_embeddings().weight):
                        w[-num_new:] = w[:-num_new].float().mean(dim=0, keepdim=True).to(w.dtype)
            pre = getattr(model_args, "pretrain_mm_mlp_adapter", None)
            if pre:
                ew = torch.load(pre, map_location="cpu")["model.embed_tokens.weight"]
                assert num_new == 2
                inp = self.get_input_embeddings().weight
                with torch.no_grad():
                    if inp.shape == ew.shape:
                        inp[-num_new:] = ew[-num_new:].to(inp)
                    elif ew.shape[0] == num_new:
                        inp[-num_new:] = ew.to(inp)
                    else:
                        raise ValueError("Unexpected embed_tokens_weight shape. Pretrained: %s. Current: %s. Numer of new tokens: %d."
                                         % (tuple(ew.shape), tuple(inp.shape), num_new))
        # (mm_use_im_patch_token alone only touches requires_grad flags that are already False here: llava_arch.py:435-440)


class LlavaLlamaForCausalLM(nn.Module, LlavaMetaForCausalLM):
    config_class = LlavaConfig

    def __init__(self, config, dtype=torch.bfloat16, device="cuda"):
        nn.Module.__init__(self)
        self.config = config
        self.model = LlavaLlamaModel(config, dtype, device)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False, dtype=dtype, device=device)
        self.lm_head.weight.requires_grad_(False)
        self._use_lora = True
        self._last_plan = None

    # -- reference surface -----------------------------------------------------------------------
    def get_model(self):
        return self.model

    def _lm_config(self):
        return self.config

    def _tokens_per_image(self):
        return self.get_vision_tower().num_patches

    def causal_lm(self):
        return self, ""

    def projector(self):
        return getattr(self.model, "mm_projector", None), "model.mm_projector."

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def get_output_embeddings(self):
        return self.lm_head

    def enable_input_require_grads(self):
        pass                                  # inputs_embeds carries grad through the projector already

    def gradient_checkpointing_enable(self, *a, **k):
        self.model.gradient_checkpointing = True

    @classmethod
    def from_pretrained(cls, path, cache_dir=None, dtype=torch.bfloat16, device="cuda", **kw):
        """Load an HF LLaVA checkpoint directory (config.json + safetensors / .bin shards)."""
        if not os.path.isdir(path):
            raise FileNotFoundError("%s is not a local checkpoint directory (no network on this path; HF hub ids must be "
                                    "downloaded beforehand)" % path)
        cfg = LlavaConfig.from_pretrained(path)
        m = cls(cfg, dtype=dtype, device=device)
        sd = _read_checkpoint(path)
        load_hf_llama_weights(m, sd, strict=True)
        proj = {k.split("mm_projector.")[1]: v for k, v in sd.items() if "mm_projector." in k}
        if proj and getattr(m.model, "mm_projector", None) is not None:
            m.model.mm_projector.load_state_dict(proj)
        return m

    def hf_state_dict(self):
        sd = hf_llama_state_dict(self)
        if getattr(self.model, "mm_projector", None) is not None:
            for k, v in self.model.mm_projector.state_dict().items():
                sd["model.mm_projector." + k] = v
        return sd

    def save_pretrained(self, path, state_dict=None):
        """Write a full checkpoint directory that from_pretrained loads: config.json + model.safetensors with the standard HF Llama
        names (the fused qkv / gate_up rows split back per projection) and the projector under `model.mm_projector.*`.  A model
        that still carries LoRA factors is refused - they would be dropped silently; merge_and_unload() first."""
        from safetensors.torch import save_file
        if state_dict is None and any(grp.A_cat is not None for layer in self.model.layers for _, grp in layer.groups()):
            raise RuntimeError("save_pretrained writes a LoRA-free checkpoint: call merge_and_unload() first (the adapter itself is "
                               "written by llava/train/train_halva.py:save_lora_outputs)")
        os.makedirs(path, exist_ok=True)
        self.config.save_pretrained(path)
        sd = self.hf_state_dict() if state_dict is None else state_dict
        save_file({k: v.detach().cpu().contiguous() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                return_dict=None):
        return self._forward_multimodal(input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, labels, use_cache,
                                        images)[0]

    def generate(self, input_ids=None, images=None, attention_mask=None, do_sample=False, temperature=None, top_p=None, num_beams=1,
                 max_new_tokens=128, use_cache=True, eos_token_id=None, pad_token_id=None, stopping_criteria=None, image_sizes=None,
                 top_k=None, generator=None, prefill_chunk=None, num_return_sequences=1, images_cd=None,
                 negative_input_ids=None, negative_attention_mask=None, cd_alpha=None, cd_beta=None, guidance_scale=None, **unused):
        """Decoding with a KV cache: the calls of the reference's hallucination benchmarks.  Greedy
        (eval_hall/model_vqa_loader.py etc.: do_sample=False, temperature=0, num_beams=1, use_cache=True), or, with do_sample=True and a
        temperature > 0 (eval_hall/model_chair_loader.py:124-130), sampling under temperature / top_k (None = 50, HF's default; 0 = off) /
        top_p (None = 1.0) with the random numbers of `generator` (a device torch.Generator; None = the default one);
        num_return_sequences = n > 1 (sampling only) gives n continuations per prompt over one prompt pass and a forked cache, rows
        b * n + i with the prompt repeated.
        Contrastive decoding (halva_amd/decode.py:contrast): images_cd= (the same ids over other images, e.g. contrast.add_diffusion_noise
        of `images`: visual contrastive decoding) or negative_input_ids= / negative_attention_mask= (another prompt: classifier-free
        guidance) adds a second row per prompt, and each token is chosen, greedily or sampled as do_sample says, from (1 + cd_alpha) *
        logits - cd_alpha * logits_cd over the tokens whose probability under the prompt as given is at least cd_beta times the largest
        (cd_alpha None = 0.5, cd_beta None = 0.1; guidance_scale=g is cd_alpha = g - 1, cd_beta = 0).  num_beams > 1 or
        num_return_sequences > 1 with it is a ValueError.
        input_ids [B, T] (IMAGE_TOKEN_INDEX marks the image; right-padded batches carry attention_mask), images [B, 3, H, W]
        (fp16 accepted).  Returns LongTensor [B, T + n]: the prompt as given, then the new tokens; a row that emitted EOS is padded
        with pad_token_id after it.  Stops when every row is done or after max_new_tokens; one host sync per step."""
        return self._generate(input_ids, images, attention_mask, do_sample, num_beams, max_new_tokens, eos_token_id, pad_token_id,
                              stopping_criteria, temperature, top_k, top_p, generator, prefill_chunk, num_return_sequences, images_cd,
                              negative_input_ids, negative_attention_mask, cd_alpha, cd_beta, guidance_scale)

    __call__ = nn.Module.__call__


def build_random_llava(cfg_kwargs, clip_kwargs, lora_r=0, lora_alpha=0, seed=0, device="cuda", max_len=2048, std=0.02,
                       share_base_from=None):
    """Random-init LLaVA of a given geometry (no checkpoints exist offline): weights N(0, std), norms 1.
    share_base_from: another model whose frozen base tensors are reused (the reference model == base of the policy)."""
    from .clip import CLIPVisionConfig
    cfg = LlavaConfig(**cfg_kwargs)
    cfg.mm_vision_tower = "random-clip"
    cfg.mm_projector_type = "mlp2x_gelu"
    cfg.mm_hidden_size = clip_kwargs["hidden_size"]
    cfg.mm_vision_select_layer = -2
    cfg.mm_vision_select_feature = "patch"
    cfg.tokenizer_model_max_length = max_len
    cfg.tokenizer_padding_side = "right"
    g = torch.Generator(device=device).manual_seed(seed)
    m = LlavaLlamaForCausalLM.__new__(LlavaLlamaForCausalLM)
    nn.Module.__init__(m)
    m.config = cfg
    m.model = LlavaLlamaModel.__new__(LlavaLlamaModel)
    m.vocab_size = cfg.vocab_size
    m._last_plan = None
    if share_base_from is None:
        LlamaModel.__init__(m.model, cfg, torch.bfloat16, device)
        m.model._dtype, m.model._device = torch.bfloat16, device
        m.model.vision_tower = CLIPVisionTower("random-clip", args=cfg, delay_load=True, config=CLIPVisionConfig(**clip_kwargs),
                                               dtype=torch.bfloat16, device=device)
        m.model.vision_tower._alloc()
        m.model.mm_projector = build_vision_projector(cfg, dtype=torch.bfloat16, device=device)
        m.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False, dtype=torch.bfloat16, device=device)
        m._use_lora = True
        with torch.no_grad():
            random_fill_(m.named_parameters(), g, std)
            vt = m.model.vision_tower
            vt.patch_w[:, 3 * clip_kwargs["patch_size"] ** 2:].zero_()
        m.model.vision_tower.requires_grad_(False)
        m.model.vision_tower.is_loaded = True
    else:
        src = share_base_from
        LlamaModel.__init__(m.model, LlavaConfig(**dict(cfg_kwargs, num_hidden_layers=0)), torch.bfloat16, device)
        m.model.config = cfg
        m.model._dtype, m.model._device = torch.bfloat16, device
        reuse_base(m.model, src.model)
        m.model.vision_tower = src.model.vision_tower
        m.model.mm_projector = FrozenProjectorView(src.model.mm_projector)
        m.lm_head = src.lm_head
        m._use_lora = False
    for p in m.parameters():
        p.requires_grad_(False)
    if lora_r:
        add_lora(m, lora_r, lora_alpha, g)
        for p in m.model.mm_projector.parameters():
            p.requires_grad_(True)
    return m
