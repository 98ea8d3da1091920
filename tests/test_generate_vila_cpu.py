"""Host-side parts of VILA generation (no GPU): the evaluation helpers of vila/mm_utils.py / vila/utils.py (the reference's
vila/mm_utils.py:205-290, vila/utils.py:111) and the adapter-name mapping and argument checks of vila/model/builder_halva.py."""
import pytest
import torch

from fake_tokenizer import FakeLlamaTokenizer


class _Tok(FakeLlamaTokenizer):
    """The fake Llama tokenizer plus batch_decode (pieces joined, the word marker back to a space, special ids dropped)."""

    def batch_decode(self, ids, skip_special_tokens=True):
        inv = {v: k for k, v in self.vocab.items()}
        out = []
        for row in ids.tolist():
            pieces = [inv.get(i, "") for i in row if not (skip_special_tokens and i in (0, 1, 2))]
            out.append("".join(pieces).replace("▁", " ").lstrip(" "))
        return out


def test_tokenizer_image_token_places_the_image_index():
    from vila.mm_utils import tokenizer_image_token
    tok = _Tok()
    mid = tokenizer_image_token("USER: <image>\nWhat is it?", tok)
    head, tail = tok("USER: ").input_ids, tok("\nWhat is it?").input_ids
    assert mid == head + [-200] + tail[1:]
    assert mid[0] == 1 and mid.count(1) == 1                       # one leading BOS
    start = tokenizer_image_token("<image>\nDescribe.", tok)
    assert start == tok("").input_ids + [-200] + tok("\nDescribe.").input_ids[1:] and start.count(-200) == 1
    end = tokenizer_image_token("Look: <image>", tok, return_tensors="pt")
    assert end.dtype == torch.long and end.tolist() == tok("Look: ").input_ids + [-200] + tok("").input_ids[1:]
    two = tokenizer_image_token("<image> and <image>", tok)
    assert two.count(-200) == 2
    assert tokenizer_image_token("a <image> b", tok, image_token_index=-7) == tok("a ").input_ids + [-7] + tok(" b").input_ids[1:]
    with pytest.raises(ValueError):
        tokenizer_image_token("x <image>", tok, return_tensors="np")


def test_model_name_from_path():
    from vila.mm_utils import get_model_name_from_path
    assert get_model_name_from_path("/ckpt/vila-13b-halva-lora/") == "vila-13b-halva-lora"
    assert get_model_name_from_path("runs/halva-vila-lora/checkpoint-400") == "halva-vila-lora_checkpoint-400"
    assert get_model_name_from_path("runs/halva-vila-lora/checkpoint-400/") == "halva-vila-lora_checkpoint-400"
    assert get_model_name_from_path("vila") == "vila"


def test_keywords_stopping_criteria():
    from transformers import StoppingCriteria
    from vila.mm_utils import KeywordsStoppingCriteria
    tok = _Tok()
    words = tok("hello world ###").input_ids[1:]                   # fills the vocabulary: [marker+hello, marker+world, marker, #, #, #]
    hello, world = words[0], words[1]
    prompt = torch.tensor([tok("USER: hi").input_ids])
    crit = KeywordsStoppingCriteria(["</s>", "###"], tok, prompt)
    assert isinstance(crit, StoppingCriteria) and crit.start_len == prompt.shape[1]
    kids = [tok("</s>").input_ids[1:], tok("###").input_ids[1:]]      # the leading BOS dropped
    assert [k.tolist() for k in crit.keyword_ids] == kids and crit.max_keyword_len == max(map(len, kids))
    assert crit(torch.tensor([[hello] + kids[0]]), None) is True       # keyword ids at the tail
    assert crit(torch.tensor([[hello] + kids[1]]), None) is True
    assert crit(torch.tensor([[hello, world]]), None) is False
    # found in the decoded text of the window although the ids at the tail differ (a one-token prompt: the window is the last
    # min(n - 1, max_keyword_len) tokens, as the reference takes it)
    crit_text = KeywordsStoppingCriteria(["world", "###"], tok, torch.tensor([[1]]))
    assert crit_text.keyword_ids[0].tolist() == [world]
    assert crit_text(torch.tensor([[hello, world, hello]]), None) is True
    assert crit_text(torch.tensor([[world, hello, hello]]), None) is False
    # batch: one bool for the whole batch, True only when every row matches
    both = torch.tensor([[hello] + kids[0], [world] + kids[0]])
    one = torch.tensor([[hello] + kids[0], [world] + [hello] * len(kids[0])])
    assert crit(both, None) is True and crit(one, None) is False


def test_disable_torch_init():
    from vila.utils import disable_torch_init
    saved = torch.nn.Linear.reset_parameters, torch.nn.LayerNorm.reset_parameters
    try:
        disable_torch_init()
        assert torch.nn.Linear.reset_parameters is not saved[0]
        assert torch.nn.LayerNorm.reset_parameters is not saved[1]
        assert torch.nn.Linear(3, 3).weight.shape == (3, 3)
    finally:
        torch.nn.Linear.reset_parameters, torch.nn.LayerNorm.reset_parameters = saved


def _tiny_vila(seed):
    from halva_amd.vila_model import build_random_vila
    llm = dict(vocab_size=64, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=64)
    sig = dict(hidden_size=144, intermediate_size=160, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=14)
    m = build_random_vila(llm, sig, lora_r=4, lora_alpha=8, seed=seed, device="cpu", max_len=64)
    with torch.no_grad():             # non-zero B factors, so that a mix-up of targets cannot go unnoticed
        for layer in m.llm.model.layers:
            for _, grp in layer.groups():
                for B in grp._Bs():
                    B.normal_(0.0, 1.0)
    return m


def test_vila_adapter_names_map_back_onto_the_lora_groups():
    """The names vila/train/train_halva.py:get_peft_state_maybe_zero_3 writes (`llm.base_model.model.model.layers...`) load into another
    model of the same geometry factor for factor; unknown names and missing factors raise."""
    import vila.train.train_halva as TV
    from vila.model.builder_halva import load_projector, load_vila_adapter, vila_adapter_state
    src, dst = _tiny_vila(1), _tiny_vila(2)
    state = TV.get_peft_state_maybe_zero_3(src, "none")
    assert state and all(k.startswith("llm.base_model.model.model.layers.") for k in state)
    assert not torch.equal(dst.llm.model.layers[0].qkv.A_cat, src.llm.model.layers[0].qkv.A_cat)
    load_vila_adapter(dst, state)
    for ls, ld in zip(src.llm.model.layers, dst.llm.model.layers):
        for (_, gs), (_, gd) in zip(ls.groups(), ld.groups()):
            assert torch.equal(gs.A_cat, gd.A_cat)
            for Bs, Bd in zip(gs._Bs(), gd._Bs()):
                assert torch.equal(Bs, Bd)
    assert TV.get_peft_state_maybe_zero_3(dst, "none").keys() == state.keys()
    with pytest.raises(KeyError):
        vila_adapter_state({"base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight": torch.zeros(1)})      # no `llm.` prefix
    with pytest.raises(KeyError):
        load_vila_adapter(dst, {"llm.base_model.model.model.mm_projector.0.weight": torch.zeros(1)})
    with pytest.raises(KeyError):
        load_vila_adapter(dst, dict(list(state.items())[1:]))                                                         # a missing factor
    # the projector of non_lora_trainables.bin
    proj = TV.get_peft_state_non_lora_maybe_zero_3(src)
    assert proj and all(k.startswith("mm_projector.") for k in proj)
    load_projector(dst, proj)
    for k, v in src.mm_projector.state_dict().items():
        assert torch.equal(dst.mm_projector.state_dict()[k], v)
    with pytest.raises(KeyError):
        load_projector(dst, {"llm.lm_head.weight": torch.zeros(1)})


def test_load_pretrained_model_refuses_what_it_cannot_load(tmp_path):
    from vila.model.builder_halva import load_pretrained_model
    with pytest.raises(NotImplementedError):
        load_pretrained_model(str(tmp_path), "vila-lora", str(tmp_path), load_8bit=True)
    with pytest.raises(NotImplementedError):
        load_pretrained_model(str(tmp_path), "vila-lora", str(tmp_path), load_4bit=True)
    with pytest.raises(FileNotFoundError):
        load_pretrained_model("Efficient-Large-Model/VILA-13b", "VILA-13b")                  # a hub name: no network
    with pytest.raises(FileNotFoundError):
        load_pretrained_model(str(tmp_path), "run-lora", "Efficient-Large-Model/VILA-13b")


def test_evaluation_imports_in_a_fresh_interpreter():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from vila.model.builder_halva import load_pretrained_model\n"
            "from vila.mm_utils import tokenizer_image_token, get_model_name_from_path, KeywordsStoppingCriteria\n"
            "from vila.utils import disable_torch_init\n"
            "from vila.model import LlavaLlamaModel\n"
            "assert hasattr(LlavaLlamaModel, 'generate')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=root))
    assert r.returncode == 0, r.stderr
