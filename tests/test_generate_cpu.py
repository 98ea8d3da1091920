"""Host-side parts of generation (no GPU): argument checks of the decode entry points, the adapter-name mapping of
llava/model/builder.py, and the eval helpers of llava/mm_utils.py / llava/utils.py."""
import pytest
import torch

from golden_util import load_json


def _lib():
    from test_cabi_symbols import _ensure_built
    _ensure_built()
    from halva_amd import hip
    return hip.load()


def test_decode_entry_points_validate_before_launching():
    lib = _lib()
    err = lambda: lib.halva_last_error()
    # halva_decode_rope_append(qkv, ldqkv, cos, sin, max_pos, kcache, vcache, lens, B, H, D, Lcap, stream)
    assert lib.halva_decode_rope_append(None, 768, 16, 16, 64, 16, 16, 16, 1, 2, 128, 8, None) == -1 and b"null pointer" in err()
    assert lib.halva_decode_rope_append(16, 576, 16, 16, 64, 16, 16, 16, 1, 2, 96, 8, None) == -1 and b"head_dim" in err()
    assert lib.halva_decode_rope_append(16, 768, 16, 16, 64, 16, 16, 16, 0, 2, 128, 8, None) == -1 and b"bad B" in err()
    assert lib.halva_decode_rope_append(16, 700, 16, 16, 64, 16, 16, 16, 1, 2, 128, 8, None) == -1 and b"row stride" in err()
    assert lib.halva_decode_rope_append(17, 768, 16, 16, 64, 16, 16, 16, 1, 2, 128, 8, None) == -1 and b"aligned" in err()
    # halva_decode_attn(q, ldq, kcache, vcache, lens, out, ld_out, ws, ws_bytes, B, H, D, Lcap, scale, stream)
    ws = lib.halva_decode_attn_ws_bytes(1, 2, 8)
    assert ws > 0 and lib.halva_decode_attn_ws_bytes(0, 2, 8) == 0
    assert lib.halva_decode_attn(16, 768, 16, None, 16, 16, 256, 16, ws, 1, 2, 128, 8, 0.0, None) == -1 and b"null pointer" in err()
    assert lib.halva_decode_attn(16, 768, 16, 16, 16, 16, 256, 16, ws, 1, 2, 64, 8, 0.0, None) == -1 and b"head_dim" in err()
    assert lib.halva_decode_attn(16, 768, 16, 16, 16, 16, 256, 16, ws, 1, 2, 128, 0, 0.0, None) == -1 and b"bad B" in err()
    assert lib.halva_decode_attn(16, 128, 16, 16, 16, 16, 256, 16, ws, 1, 2, 128, 8, 0.0, None) == -1 and b"q row stride" in err()
    assert lib.halva_decode_attn(16, 768, 16, 16, 16, 16, 128, 16, ws, 1, 2, 128, 8, 0.0, None) == -1 and b"out row stride" in err()
    assert lib.halva_decode_attn(16, 768, 16, 16, 16, 16, 256, 16, ws - 4, 1, 2, 128, 8, 0.0, None) == -1 and b"workspace" in err()
    assert lib.halva_decode_attn_kc() == 256
    # the measurement entry takes the chunk explicitly: 64, 128 or 256 keys
    assert lib.halva_decode_attn_chunked(16, 768, 16, 16, 16, 16, 256, 16, 1 << 20, 1, 2, 128, 8, 0.0, 100, None) == -1 and b"chunk" in err()


def test_workspace_size_follows_the_chunk_count():
    lib = _lib()
    kc = lib.halva_decode_attn_kc()
    for B, H, L in ((1, 2, 1), (3, 32, kc), (3, 32, kc + 1), (16, 32, 4097)):
        assert lib.halva_decode_attn_ws_bytes(B, H, L) == B * H * ((L + kc - 1) // kc) * 130 * 4


def _tiny(seed):
    from halva_amd.llava_model import build_random_llava
    d = load_json("peft_state_names.json")
    vis = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=14, layer_norm_eps=1e-5)
    m = build_random_llava(d["llama_cfg"], vis, lora_r=d["lora_r"], lora_alpha=8, seed=seed, device="cpu", max_len=64)
    with torch.no_grad():             # non-zero B factors, so that a mix-up of targets cannot go unnoticed
        for layer in m.model.layers:
            for _, grp in layer.groups():
                for B in grp._Bs():
                    B.normal_(0.0, 1.0)
    return m, d


def test_peft_names_map_back_onto_the_lora_groups():
    """load_peft_state inverts get_peft_state_maybe_zero_3: the adapter written from one model, loaded into another of the same
    geometry, reproduces every factor; the names are those pinned in tests/golden/peft_state_names.json."""
    import llava.train.train_halva as TH
    from llava.model.builder import load_peft_state, peft_name_to_target
    src, d = _tiny(1)
    dst, _ = _tiny(2)
    state = TH.get_peft_state_maybe_zero_3(src, "none")
    assert list(state) == list(d["adapter_model_bin"])
    for name in d["adapter_model_bin"]:
        i, sub, target, ab = peft_name_to_target(name)
        assert name == "base_model.model.model.layers.%d.%s.%s.lora_%s.weight" % (i, sub, target, ab)
    for name in d["lora_state"]:
        assert peft_name_to_target(name)[:3] == peft_name_to_target(name.replace(".default", ""))[:3]
    assert not torch.equal(dst.model.layers[0].qkv.A_cat, src.model.layers[0].qkv.A_cat)
    load_peft_state(dst, state)
    for ls, ld in zip(src.model.layers, dst.model.layers):
        for (_, gs), (_, gd) in zip(ls.groups(), ld.groups()):
            assert torch.equal(gs.A_cat, gd.A_cat)
            for Bs, Bd in zip(gs._Bs(), gd._Bs()):
                assert torch.equal(Bs, Bd)
    assert TH.get_peft_state_maybe_zero_3(dst, "none").keys() == state.keys()
    with pytest.raises(KeyError):
        load_peft_state(dst, {k: v for k, v in list(state.items())[1:]})        # a missing factor is an error
    with pytest.raises(KeyError):
        peft_name_to_target("base_model.model.model.mm_projector.0.weight")


def test_model_name_from_path():
    from llava.mm_utils import get_model_name_from_path
    assert get_model_name_from_path("/ckpt/llava-v1.5-7b-halva-lora/") == "llava-v1.5-7b-halva-lora"
    assert get_model_name_from_path("runs/halva-lora/checkpoint-400") == "halva-lora_checkpoint-400"
    assert get_model_name_from_path("halva") == "halva"


class _Proc:
    """The CLIPImageProcessor surface process_images uses (preprocess / __call__ -> pixel_values): nearest resize, scale to [0, 1]."""
    image_mean = [0.5, 0.25, 0.0]

    def __init__(self, size=8):
        self.size = size

    def preprocess(self, img, return_tensors="pt"):
        import numpy as np
        from PIL import Image
        a = np.asarray(img.resize((self.size, self.size), Image.NEAREST)).astype("float32") / 255.0
        return {"pixel_values": torch.from_numpy(a).permute(2, 0, 1)[None]}

    def __call__(self, images, return_tensors="pt"):
        return {"pixel_values": torch.cat([self.preprocess(im)["pixel_values"] for im in images])}


def test_process_images_pads_to_square_in_the_mean_colour():
    from PIL import Image
    from llava.mm_utils import process_images
    import types
    ims = [Image.new("RGB", (4, 2), (255, 255, 255)), Image.new("RGB", (6, 6), (0, 0, 0))]
    out = process_images(ims, _Proc(), types.SimpleNamespace(image_aspect_ratio="pad"))
    assert out.shape == (2, 3, 8, 8)
    # the 4 x 2 white image sits in the middle rows of a 4 x 4 canvas of the mean colour (127, 63, 0)
    assert torch.allclose(out[0, :, 0, 0], torch.tensor([127, 63, 0]) / 255.0)
    assert torch.allclose(out[0, :, 4, 4], torch.ones(3))
    plain = process_images(ims, _Proc(), types.SimpleNamespace())
    assert plain.shape == (2, 3, 8, 8) and torch.allclose(plain[0, :, 0, 0], torch.ones(3))


def test_disable_torch_init():
    from llava.utils import disable_torch_init
    saved = torch.nn.Linear.reset_parameters, torch.nn.LayerNorm.reset_parameters
    try:
        disable_torch_init()
        lin = torch.nn.Linear(3, 3)          # no initialisation: whatever the allocator held
        assert lin.weight.shape == (3, 3)
        assert torch.nn.Linear.reset_parameters is not saved[0]
    finally:
        torch.nn.Linear.reset_parameters, torch.nn.LayerNorm.reset_parameters = saved

