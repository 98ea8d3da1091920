#!/usr/bin/env python3
"""Fold a trained LoRA run into its base model and write the result as a plain full checkpoint: load_pretrained_model with the adapter
(merge_lora=True: what the reference's loader does before evaluation, llava/model/builder.py:70-71), then save_pretrained.  Local paths
only.

    python tools/merge_lora_weights.py --model-path RUN --model-base BASE --save-model-path OUT

RUN holds adapter_model.bin, non_lora_trainables.bin, adapter_config.json and config.json (llava/train/train_halva.py:save_lora_outputs);
BASE is the HF LLaVA directory the run was trained from.  OUT gets config.json (the run's settings) and model.safetensors: the standard HF
Llama names with every projection's weight bf16(W + alpha / r * B A) (halva_lora_merge: fp32 accumulation in a fixed order, one rounding -
the same bytes on every run), the run's projector under model.mm_projector.*, no LoRA tensor.  OUT loads with
llava.model.builder.load_pretrained_model(OUT, None, name) - or with any runtime that reads HF LLaVA checkpoints - without LoRA code.
The tokenizer files of BASE, if it has any, are copied alongside.
"""
import argparse
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_TOKENIZER_FILES = ("tokenizer_config.json", "tokenizer.model", "tokenizer.json", "special_tokens_map.json", "added_tokens.json")


def merge_lora(model_path, model_base, save_model_path, device="cuda"):
    from llava.model.builder import load_pretrained_model
    name = os.path.basename(os.path.normpath(model_path))
    if "lora" not in name.lower():
        name += "-lora"          # (the loader tells a LoRA run from a full checkpoint by its name, as the reference does)
    _, model, _, _ = load_pretrained_model(model_path, model_base, name, device=device, merge_lora=True)
    model.save_pretrained(save_model_path)
    for f in _TOKENIZER_FILES:
        if os.path.exists(os.path.join(model_base, f)):
            shutil.copy(os.path.join(model_base, f), os.path.join(save_model_path, f))
    return model


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model-path", required=True)
    ap.add_argument("--model-base", required=True)
    ap.add_argument("--save-model-path", required=True)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    merge_lora(a.model_path, a.model_base, a.save_model_path, a.device)
    print("merged checkpoint written to %s" % a.save_model_path)


if __name__ == "__main__":
    main()
