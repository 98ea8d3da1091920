"""One sha256 per item of the Python layer between the C ABI and the step engine, on tiny geometries with fixed seeds: run it on two
commits on the same GPU and compare the lines - a refactor of halva_amd/{multimodal,llava_model,vila_model,clip,siglip,kernels,dpa}.py
must leave every line as it was.

    python tools/model_surface_digest.py [--save unstable.pt]

Lines that start with `~` hold bias and LayerNorm-parameter gradients: they pass through float atomicAdd (colsum_kernel,
layernorm_bwd_params_kernel) and are not run-to-run stable, so each also carries its max |difference| to an fp32 torch restatement.
--save writes those tensors to a file, for the spread between two runs.  Single process, well under a minute.
"""
import argparse
import hashlib
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

LLM = dict(vocab_size=160, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
           max_position_embeddings=256, rms_norm_eps=1e-5, pad_token_id=0)
CLIP = dict(hidden_size=128, intermediate_size=192, num_hidden_layers=3, num_attention_heads=2, image_size=28, patch_size=14,
            layer_norm_eps=1e-5)
SIGLIP = dict(hidden_size=144, intermediate_size=160, num_hidden_layers=3, num_attention_heads=2, image_size=48, patch_size=14)
UNSTABLE = {}


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        if isinstance(t, torch.Tensor):
            t = t.detach().cpu().contiguous()
            h.update(str((t.dtype, tuple(t.shape))).encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        else:
            h.update(repr(t).encode())
    return h.hexdigest()


def item(name, fn):
    """Print `name digest`; an exception is part of the surface too (its type and message are the item)."""
    try:
        out = fn()
    except Exception as e:          # noqa: BLE001
        out = "raised %s: %s" % (type(e).__name__, e)
    print("%s %s" % (name, out if isinstance(out, str) else sha(*out)), flush=True)


def unstable(name, got, want):
    UNSTABLE[name] = got.detach().float().cpu()
    print("~%s %s maxabs_to_fp32_torch=%.3e" % (name, sha(got), float((got.float() - want.float()).abs().max())), flush=True)


def params(m):
    out = []
    for n, p in m.named_parameters():
        out += [n, p.requires_grad, p]
    return out


def models():
    from halva_amd.llava_model import build_random_llava
    from halva_amd.vila_model import build_random_vila
    lp = build_random_llava(LLM, CLIP, lora_r=8, lora_alpha=16, seed=3, device="cuda", max_len=192)
    lr = build_random_llava(LLM, CLIP, seed=3, device="cuda", max_len=192, share_base_from=lp)
    vp = build_random_vila(LLM, SIGLIP, lora_r=8, lora_alpha=16, seed=4, device="cuda", max_len=192)
    vr = build_random_vila(LLM, SIGLIP, seed=4, device="cuda", max_len=192, share_base_from=vp)
    for name, m in (("llava.policy", lp), ("llava.reference", lr), ("vila.policy", vp), ("vila.reference", vr)):
        item("params." + name, lambda m=m: params(m))
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():           # non-zero B factors: the LoRA path must matter to every later item
        for layers in (lp.model.layers, vp.llm.model.layers):
            for layer in layers:
                for _, grp in layer.groups():
                    for n in grp.names:
                        getattr(grp, n).lora_B["default"].weight.normal_(0.0, 0.02, generator=g)
    return lp, lr, vp, vr


def towers(lp, vp):
    g = torch.Generator().manual_seed(6)
    for name, vt, hw in (("clip", lp.model.vision_tower, 28), ("siglip", vp.vision_tower, 48)):
        im = torch.randn(3, 3, hw, hw, generator=g).to("cuda", torch.bfloat16)
        keep = vt.select_feature
        for sel in ("patch", "cls_patch"):
            vt.select_feature = sel
            item("tower.%s.%s" % (name, sel), lambda: [vt(im)])
        vt.select_feature = keep


def _downsample_ref(x):
    """[n, g*g, c] -> [n, G*G, 4c] as halva_amd/csrc/vision.hip states it: out[n, b*G + a, (f*2 + e)*c + ch] = x[n, (2a + f)*g + 2b + e, ch]."""
    n, s, c = x.shape
    g = int(s ** 0.5)
    G = (g + 1) // 2
    xp = x.new_zeros(n, 2 * G, 2 * G, c)
    xp[:, :g, :g] = x.view(n, g, g, c)
    return xp.view(n, G, 2, G, 2, c).permute(0, 3, 1, 2, 4, 5).reshape(n, G * G, 4 * c)


def projector_reference(kind, proj, x, dy):
    """fp32 torch restatement on the same bf16 inputs -> (y, {parameter name: gradient})."""
    prm = {n: p.detach().float().requires_grad_(True) for n, p in proj.named_parameters()}
    h = x.float()
    if kind == "mlp_downsample":
        h = _downsample_ref(h)
        h = F.layer_norm(h, (h.shape[-1],), prm["layers.1.weight"], prm["layers.1.bias"], proj.layers[1].eps)
        lin = [("layers.2.", True), ("layers.4.", False)]
    elif kind == "linear":
        lin = [("", False)]
    else:
        depth = len(prm) // 2
        lin = [("%d." % (2 * i), i + 1 < depth) for i in range(depth)]
    for pre, act in lin:
        h = F.linear(h, prm[pre + "weight"], prm[pre + "bias"])
        if act:
            h = F.gelu(h)
    h.backward(dy.float())
    return h.detach(), {n: p.grad for n, p in prm.items()}


def projectors():
    from halva_amd.clip import build_vision_projector
    from halva_amd.vila_model import MultimodalProjector
    cfg = SimpleNamespace(mm_hidden_size=64, hidden_size=128)
    for kind in ("linear", "mlp2x_gelu", "mlp3x_gelu", "mlp_downsample"):
        for sink in (False, True):
            g = torch.Generator(device="cuda").manual_seed(7)
            if kind == "mlp_downsample":
                cfg.mm_hidden_size = 32
                proj = MultimodalProjector(kind, cfg, device="cuda")
            else:
                cfg.mm_hidden_size, cfg.mm_projector_type = 64, kind
                proj = build_vision_projector(cfg, device="cuda")
            with torch.no_grad():
                for n, p in proj.named_parameters():
                    p.normal_(0.0, 0.1, generator=g)
                    if n == "layers.1.weight":
                        p.add_(1.0)
            x = torch.randn(2, 9, cfg.mm_hidden_size, device="cuda", generator=g).bfloat16()
            for p in proj.parameters():
                if sink:
                    p.main_grad, p.grad_sink = torch.zeros(p.shape, dtype=torch.float32, device="cuda"), True
            y = proj(x)
            dy = torch.randn(y.shape, device="cuda", generator=g).bfloat16()
            y.backward(dy)
            y_ref, g_ref = projector_reference(kind, proj, x, dy)
            tag = "projector.%s.%s" % (kind, "sink" if sink else "autograd")
            item(tag + ".output", lambda: [y])
            for n, p in proj.named_parameters():
                if sink:
                    assert p.grad is None
                got = p.main_grad if sink else p.grad
                if p.ndim == 2:
                    item("%s.grad.%s" % (tag, n), lambda: [got])
                else:
                    unstable("%s.grad.%s" % (tag, n), got, g_ref[n])


def _prompts(image_tokens):
    g = torch.Generator().manual_seed(8)
    rows = [torch.randint(3, 160, (n,), generator=g) for n in (19, 11, 26)]
    for r in rows:
        r[0] = 1
        if image_tokens:
            r[4] = -200
    T = max(len(r) for r in rows)
    ids = torch.zeros(len(rows), T, dtype=torch.long)
    mask = torch.zeros(len(rows), T, dtype=torch.bool)
    for i, r in enumerate(rows):
        ids[i, :len(r)], mask[i, :len(r)] = r, True
    return ids, mask


def forward_and_generate(lp, vp):
    g = torch.Generator().manual_seed(9)
    for name, m, hw in (("llava", lp, 28), ("vila", vp, 48)):
        images = torch.randn(3, 3, hw, hw, generator=g).to("cuda", torch.bfloat16)
        ids, mask = _prompts(True)
        labels = ids.clone()
        labels[:, :6] = -100
        labels[~mask] = -100
        for tag, lab in (("labels", labels), ("all_ignored", torch.full_like(labels, -100))):
            def run():
                with torch.no_grad():
                    out = m.forward(input_ids=ids.cuda(), attention_mask=mask.cuda(), labels=lab.cuda(), images=images)
                return [out.logits, out.loss, sorted(vars(out))]
            item("forward.%s.%s" % (name, tag), run)
        item("generate.%s.images" % name,
             lambda: [m.generate(ids, images=images, attention_mask=mask, max_new_tokens=8, eos_token_id=[])])
        tids, tmask = _prompts(False)
        item("generate.%s.text_only" % name, lambda: [m.generate(tids, attention_mask=tmask, max_new_tokens=8, eos_token_id=[])])
        item("generate.%s.left_padded" % name,
             lambda: [m.generate(ids.flip(1), images=images, attention_mask=mask.flip(1), max_new_tokens=2, eos_token_id=[])])
        item("generate.%s.image_tokens_without_images" % name, lambda: [m.generate(ids, attention_mask=mask, max_new_tokens=2)])


def engine(name, pol, ref, hw, vila):
    import bench
    from halva_amd import dpa
    flat = dpa.FlatTrainables(dpa.trainable_named_parameters(pol))
    dpa.bind_model(flat, pol)
    dpa.set_grad_sink(pol, True)
    batch = bench.synthetic_batch(3, 10, resp_len=60, vocab=160, image=hw, images_per_sample=1 if vila else None, n_phrases=1)
    eng = dpa.DPAEngine(pol, ref, 0.4, pairs_per_group=2, ref_rows_per_group=2)
    loss = eng.loss(batch, backward=True)
    torch.cuda.synchronize()
    item("engine.%s.spec" % name, lambda: repr(sorted(vars(dpa.model_spec(pol)).items())))
    item("engine.%s.loss" % name, lambda: [loss, eng.last_parts["alignment"], eng.last_parts["divergence"]])
    item("engine.%s.names" % name, lambda: [flat.names, sorted(flat.no_decay)])
    stable = [i for i, n in enumerate(flat.names) if n not in flat.no_decay]
    item("engine.%s.grads" % name, lambda: [flat.grad[flat.offsets[i]:flat.offsets[i + 1]] for i in stable])
    for i, n in enumerate(flat.names):
        if n in flat.no_decay:
            got = flat.grad[flat.offsets[i]:flat.offsets[i + 1]]
            UNSTABLE["engine.%s.grad.%s" % (name, n)] = got.detach().float().cpu()
            print("~engine.%s.grad.%s %s maxabs=%.3e" % (name, n, sha(got), float(got.abs().max())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", default=None, help="write the run-to-run unstable tensors here")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lp, lr, vp, vr = models()
    towers(lp, vp)
    projectors()
    forward_and_generate(lp, vp)
    engine("llava", lp, lr, 28, False)
    engine("vila", vp, vr, 48, True)
    torch.cuda.synchronize()
    if args.save:
        os.makedirs(os.path.dirname(os.path.abspath(args.save)), exist_ok=True)
        torch.save(UNSTABLE, args.save)


if __name__ == "__main__":
    main()
