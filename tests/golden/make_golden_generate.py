#!/usr/bin/env python3
"""Generate tests/golden/generate_d128.npz: greedy decoding of the REFERENCE's LlavaLlamaForCausalLM (CPU, fp32) on the weights of
dpa_step_d128_init.npz (2 layers, 2 heads x 128, vocab 160) with its LoRA factors merged (W + (alpha / r) B A, as make_golden.py:lora_merge
builds the policy), for 3 prompts with one image each and different text lengths.

Each of the 24 steps runs the reference's own forward on the whole prefix (no cache, use_cache=False): the arithmetic that a cached
`generate(use_cache=True)` is defined to match, without HF generation internals.  Only inputs and outputs are stored: the prompt ids,
the generated ids, every step's last-row logits and their top-1 / top-2 gap.

Usage:  python tests/golden/make_golden_generate.py          (runs where the reference tree is mounted, like make_golden.py)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (imports the reference the same way)

PROMPT_LENS = (20, 33, 47)
STEPS = 24


def _bits_to_f32(a):
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.astype(np.uint32) << 16).view(torch.float32)
    return torch.from_numpy(np.array(a, dtype=np.float32))


def build_reference(z):
    llama = json.loads(bytes(z["llama_cfg"]).decode())
    vis = json.loads(bytes(z["clip_cfg"]).decode())
    tower = MG.build_vision_tower(41, vis, bf16_round=True)
    tower.vision_tower.load_state_dict({k[len("clip."):]: _bits_to_f32(z[k]) for k in z.files if k.startswith("clip.")}, strict=False)
    m = MG.build_llava(310, tower, max_len=int(z["max_len"]), tiny=llama, vis=vis, bf16_round=True, std=0.02)
    sd = {k[len("base."):]: _bits_to_f32(z[k]) for k in z.files if k.startswith("base.")}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("vision_tower" in k or "rotary" in k for k in missing), missing
    r, alpha = int(z["lora_cfg"][0]), float(z["lora_cfg"][1])
    mods = dict(m.named_modules())
    with torch.no_grad():
        for k in z.files:
            if k.startswith("lora.") and k.endswith(".A"):
                name = k[len("lora."):-len(".A")]
                A, Bm = _bits_to_f32(z[k]), _bits_to_f32(z["lora." + name + ".B"])
                mods[name].weight.add_((alpha / r) * (Bm @ A))
    m.eval()
    return m


@torch.no_grad()
def greedy(m, prompt, image):
    ids = prompt.clone()
    toks, logits, gaps = [], [], []
    for _ in range(STEPS):
        out = m(input_ids=ids[None], images=image[None], use_cache=False)
        lg = out.logits[0, -1].float()
        top2 = lg.topk(2).values
        nxt = int(lg.argmax())
        toks.append(nxt)
        logits.append(lg.numpy())
        gaps.append(float(top2[0] - top2[1]))
        ids = torch.cat([ids, torch.tensor([nxt], dtype=ids.dtype)])
    return np.array(toks, np.int64), np.stack(logits), np.array(gaps, np.float32)


def main():
    torch.set_num_threads(4)
    z = np.load(os.path.join(HERE, "dpa_step_d128_init.npz"))
    m = build_reference(z)
    ids = torch.from_numpy(z["batch.input_ids"][:3].astype(np.int64))
    images = torch.from_numpy(z["batch.images"][:3].astype(np.float32))
    packs = {"prompt_lens": np.array(PROMPT_LENS, np.int64)}
    for i, n in enumerate(PROMPT_LENS):
        toks, logits, gaps = greedy(m, ids[i, :n], images[i])
        packs["prompt.%d" % i] = ids[i, :n].numpy()
        packs["tokens.%d" % i] = toks
        packs["logits.%d" % i] = logits
        packs["gap.%d" % i] = gaps
        print("   prompt %d (%d ids): tokens %s, min top-2 gap %.3e" % (i, n, toks.tolist(), float(gaps.min())))
    MG.save_npz("generate_d128.npz", **packs)


if __name__ == "__main__":
    main()
