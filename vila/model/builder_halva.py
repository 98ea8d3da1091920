"""load_pretrained_model of the reference's VILA evaluation (vila/model/builder_halva.py) for the two kinds of output HALVA-VILA training
writes, local paths only.  The argument order is the reference's (model_path, model_name, model_base), not the llava twin's.

  * LoRA (`lora` in model_name, model_base given): model_base is a VILA checkpoint directory (config.json with llm / vision_tower /
    mm_projector); model_path holds adapter_model.bin, non_lora_trainables.bin and adapter_config.json as
    vila/train/train_halva.py:save_lora_outputs writes them.  The projector comes from non_lora_trainables.bin; the factors of `.llm`'s
    adapter (`llm.base_model.model.model.layers.<i>.<sub>.<target>.lora_<A|B>.weight`) go back onto the LoraGroup factors and stay
    unmerged (generation then computes what training computed); with merge_lora=True they are folded into the base weights after
    loading, as the reference does with peft (`Merging LoRA weights...`, merge_and_unload()).  No peft is needed.
  * otherwise: a full VILA checkpoint directory.

Returns (tokenizer, model, image_processor, context_len), the reference's tuple.  The tokenizer is None when the checkpoint's llm
directory holds no tokenizer files.
"""
import json
import os

import torch

from halva_amd.llama import add_lora
from halva_amd.vila_model import VilaConfig, VilaLlavaLlamaModel
from llava.model.builder import _local_dir, load_peft_state

_LLM_PREFIX = "llm."


def vila_adapter_state(state):
    """adapter_model.bin of a VILA run -> the llava twin's PEFT naming (`base_model.model.model.layers...`), which
    llava.model.builder.load_peft_state maps onto the LoraGroup factors.  A name outside `llm.` raises KeyError."""
    out = {}
    for name, t in state.items():
        if not name.startswith(_LLM_PREFIX):
            raise KeyError("not a LoRA factor of the VILA `.llm` adapter: %s" % name)
        out[name[len(_LLM_PREFIX):]] = t
    return out


def load_vila_adapter(model, state):
    """Copy a VILA adapter_model.bin state into the model's LoRA factors (every factor must be present; the names are checked)."""
    return load_peft_state(model, vila_adapter_state(state))


def load_projector(model, state):
    """non_lora_trainables.bin ({`mm_projector.<name>`: tensor}) -> model.mm_projector (strict)."""
    proj = {k[len("mm_projector."):]: v for k, v in state.items() if k.startswith("mm_projector.")}
    if len(proj) != len(state):
        raise KeyError("non_lora_trainables.bin holds names outside mm_projector: %s" % sorted(set(state) - {"mm_projector." + k for k in proj}))
    if proj:
        model.mm_projector.load_state_dict(proj)


def _build(path, dev):
    config = VilaConfig.from_pretrained(path)
    config.resume_path = path
    return VilaLlavaLlamaModel(config, device=dev)


def load_pretrained_model(model_path, model_name, model_base=None, load_8bit=False, load_4bit=False, device_map="auto", device="cuda",
                          merge_lora=False, **kwargs):
    if load_8bit or load_4bit:
        raise NotImplementedError("8-bit / 4-bit loading is not supported: the model runs in bf16")
    dev = device
    _local_dir(model_path, "model_path")
    if "lora" in model_name.lower() and model_base is not None:
        _local_dir(model_base, "model_base")
        model = _build(model_base, dev)
        with open(os.path.join(model_path, "adapter_config.json")) as f:
            acfg = json.load(f)
        add_lora(model.llm, int(acfg["r"]), float(acfg["lora_alpha"]))
        for layer in model.llm.model.layers:
            for _, grp in layer.groups():
                grp.weight_cat_t = None          # (the transposed copy serves the training backward only)
        nl = os.path.join(model_path, "non_lora_trainables.bin")
        if os.path.exists(nl):
            load_projector(model, torch.load(nl, map_location="cpu"))
        load_vila_adapter(model, torch.load(os.path.join(model_path, "adapter_model.bin"), map_location="cpu"))
        if merge_lora:
            print("Merging LoRA weights...")
            model.merge_and_unload()
    else:
        model = _build(model_path, dev)
    for p in model.parameters():
        p.requires_grad_(False)
    model.eval()
    image_processor = None
    vt = model.get_vision_tower()
    if vt is not None:
        if not vt.is_loaded:
            vt.load_model()
        image_processor = getattr(vt, "image_processor", None)
    lc = model.llm.config
    context_len = getattr(model.config, "max_sequence_length", lc.max_sequence_length) if hasattr(lc, "max_sequence_length") else 2048
    return model.tokenizer, model, image_processor, context_len
