"""load_pretrained_model of the reference (llava/model/builder.py) for the two kinds of output HALVA training writes, local paths only:

  * LoRA (`lora` in model_name, model_base given): model_base is an HF LLaVA directory; model_path holds adapter_model.bin,
    non_lora_trainables.bin, adapter_config.json and config.json as llava/train/train_halva.py:save_lora_outputs writes them.  The
    PEFT-named factors go back onto the LoraGroup factors (the inverse of get_peft_state_maybe_zero_3) and stay unmerged: generation
    computes exactly what training computed.  With merge_lora=True they are folded into the base weights after loading, as the
    reference does (`Merging LoRA weights...`, model.merge_and_unload()): the model then runs LoRA-free, and tools/merge_lora_weights.py
    writes it out as a full checkpoint.  No peft is needed.
  * a full checkpoint: LlavaLlamaForCausalLM.from_pretrained(model_path).

Returns (tokenizer, model, image_processor, context_len).  The tokenizer is None when the tokenizer directory holds no tokenizer files.
"""
import json
import os
import re

import torch

from halva_amd.llama import add_lora
from halva_amd.llava_model import LlavaConfig, LlavaLlamaForCausalLM

_PEFT_NAME = re.compile(r"^base_model\.model\.model\.layers\.(\d+)\.(self_attn|mlp)\.([a-z_]+)\.lora_(A|B)(?:\.default)?\.weight$")


def peft_name_to_target(name):
    """`base_model.model.model.layers.<i>.<sub>.<target>.lora_<A|B>.weight` -> (i, sub, target, "A" | "B")."""
    m = _PEFT_NAME.match(name)
    if m is None:
        raise KeyError("not a LoRA factor name of adapter_model.bin: %s" % name)
    return int(m.group(1)), m.group(2), m.group(3), m.group(4)


def _group_of(layer, sub, target):
    for s, grp in layer.groups():
        if s == sub and target in grp.names:
            return grp
    raise KeyError("no LoRA target %s.%s in the decoder layer" % (sub, target))


def load_peft_state(model, state):
    """Copy an adapter_model.bin state ({PEFT name: tensor}) into the model's LoRA factors (A into its rows of the group's A_cat, B into
    the target's lora_B).  Every factor of the model must be present; the fused tails refresh on the next forward."""
    layers = model.get_model().layers
    seen = set()
    with torch.no_grad():
        for name, t in state.items():
            i, sub, target, ab = peft_name_to_target(name)
            grp = _group_of(layers[i], sub, target)
            if grp.A_cat is None:
                raise ValueError("the model has no LoRA factors attached (add_lora first)")
            g, r = grp.names.index(target), grp.r
            dst = grp.A_cat.data[g * r:(g + 1) * r] if ab == "A" else getattr(grp, target).lora_B["default"].weight.data
            if tuple(dst.shape) != tuple(t.shape):
                raise ValueError("%s: shape %s, the model's factor is %s" % (name, tuple(t.shape), tuple(dst.shape)))
            dst.copy_(t)
            seen.add((i, sub, target, ab))
        for i, layer in enumerate(layers):
            for sub, grp in layer.groups():
                for target in grp.names:
                    for ab in "AB":
                        if grp.A_cat is not None and (i, sub, target, ab) not in seen:
                            raise KeyError("adapter_model.bin has no lora_%s for layer %d %s.%s" % (ab, i, sub, target))
    return model


def _strip_prefix(state):
    """non_lora_trainables.bin keys -> `model.mm_projector.*` (reference builder.py: drop `base_model.`, then a doubled `model.`)."""
    out = {(k[len("base_model."):] if k.startswith("base_model.") else k): v for k, v in state.items()}
    if any(k.startswith("model.model.") for k in out):
        out = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in out.items()}
    return out


def _load_projector(model, state):
    proj = {k.split("mm_projector.", 1)[1]: v for k, v in _strip_prefix(state).items() if "mm_projector." in k}
    if proj:
        model.get_model().mm_projector.load_state_dict(proj)


def _load_tokenizer(path):
    if path is None or not any(os.path.exists(os.path.join(path, f)) for f in ("tokenizer_config.json", "tokenizer.model", "tokenizer.json")):
        return None
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(path, use_fast=False, local_files_only=True)


def _local_dir(path, what):
    if path is None or not os.path.isdir(path):
        raise FileNotFoundError("%s %r is not a local directory (models are loaded from local paths only)" % (what, path))
    return path


def _base_with_config(model_base, model_path, dev):
    """The base weights with the trained run's config.json (its settings - image_aspect_ratio, tokenizer_model_max_length, .. - apply;
    the geometry must be the base's)."""
    model = LlavaLlamaForCausalLM.from_pretrained(model_base, device=dev)
    cfg = LlavaConfig.from_pretrained(model_path)
    for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "vocab_size"):
        if getattr(cfg, k) != getattr(model.config, k):
            raise ValueError("%s: %s in %s, %s in the base model %s" % (k, getattr(cfg, k), model_path, getattr(model.config, k), model_base))
    model.config.__dict__.update({k: v for k, v in cfg.__dict__.items() if k != "mm_vision_tower" or not hasattr(model.config, k)})
    return model


def load_pretrained_model(model_path, model_base, model_name, load_8bit=False, load_4bit=False, device_map="auto", device="cuda",
                          merge_lora=False, **kwargs):
    if load_8bit or load_4bit:
        raise NotImplementedError("8-bit / 4-bit loading is not supported: the model runs in bf16")
    dev = device
    _local_dir(model_path, "model_path")
    if "lora" in model_name.lower() and model_base is not None:
        _local_dir(model_base, "model_base")
        model = _base_with_config(model_base, model_path, dev)
        with open(os.path.join(model_path, "adapter_config.json")) as f:
            acfg = json.load(f)
        add_lora(model, int(acfg["r"]), float(acfg["lora_alpha"]))
        for layer in model.get_model().layers:
            for _, grp in layer.groups():
                grp.weight_cat_t = None          # (the transposed copy serves the training backward only)
        _load_projector(model, torch.load(os.path.join(model_path, "non_lora_trainables.bin"), map_location="cpu"))
        load_peft_state(model, torch.load(os.path.join(model_path, "adapter_model.bin"), map_location="cpu"))
        if merge_lora:
            print("Merging LoRA weights...")
            model.merge_and_unload()
        tokenizer = _load_tokenizer(model_base)
    elif model_base is not None:
        # the projector alone over a base model (mm_projector.bin of a pretraining stage)
        _local_dir(model_base, "model_base")
        model = _base_with_config(model_base, model_path, dev)
        _load_projector(model, torch.load(os.path.join(model_path, "mm_projector.bin"), map_location="cpu"))
        tokenizer = _load_tokenizer(model_base)
    else:
        model = LlavaLlamaForCausalLM.from_pretrained(model_path, device=dev)
        tokenizer = _load_tokenizer(model_path)
    for p in model.parameters():
        p.requires_grad_(False)
    image_processor = None
    vt = model.get_vision_tower()
    if vt is not None:
        if not vt.is_loaded:
            vt.load_model()
        image_processor = vt.image_processor
    context_len = getattr(model.config, "max_sequence_length", 2048)
    return tokenizer, model, image_processor, context_len
