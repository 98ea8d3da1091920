"""reference vila/mm_utils.py:150-290 - the pieces HallDataset and the VILA evaluation scripts (eval_hall_vila/*) use.
tokenizer_image_token and get_model_name_from_path are the same in both reference trees: the llava twin's are reused."""
import os

import torch
from PIL import Image

from llava.mm_utils import get_model_name_from_path, tokenizer_image_token  # noqa: F401

try:
    from transformers import StoppingCriteria as _StoppingCriteria
except ImportError:             # (only the isinstance relation to HF's base class is lost)
    _StoppingCriteria = object


def _expand2square(img, fill):
    w, h = img.size
    if w == h:
        return img
    side = max(w, h)
    canvas = Image.new(img.mode, (side, side), fill)
    canvas.paste(img, ((side - w) // 2, (side - h) // 2))
    return canvas


def process_image(image_file, data_args, image_folder):
    """mm_utils.py:150-193.  'resize': PIL-resize to the processor's square size first; 'pad': expand to a square filled
    with the processor mean; then the tower's own preprocessing (SigLIP: resize + rescale + normalise)."""
    processor = data_args.image_processor
    if isinstance(image_file, str):
        path = os.path.join(image_folder, image_file) if image_folder is not None else image_file
        image = Image.open(path).convert("RGB")
    else:
        image = image_file
    if data_args.image_aspect_ratio == "resize":
        size = processor.crop_size if hasattr(processor, "crop_size") and processor.crop_size else processor.size
        image = image.resize((size["height"], size["width"]))
    if data_args.image_aspect_ratio == "pad":
        image = _expand2square(image, tuple(int(x * 255) for x in processor.image_mean))
    return processor.preprocess(image, return_tensors="pt")["pixel_values"][0]


def process_images(images, image_processor, model_cfg):
    model_cfg.image_processor = image_processor
    out = [process_image(im, model_cfg, None) for im in images]
    if all(x.shape == out[0].shape for x in out):
        out = torch.stack(out, dim=0)
    return out


def is_gemma_tokenizer(tokenizer):
    return "gemma" in tokenizer.__class__.__name__.lower()


class KeywordsStoppingCriteria(_StoppingCriteria):
    """mm_utils.py:246-290: stop once every row ends in one of the keywords, matched on the token ids at the tail or found in the
    decoded text of the last few tokens.  __call__ returns ONE bool for the whole batch (all rows must match).  start_len is the
    prompt's length, as the reference records it; generate() hands over the new tokens only (HF does so for inputs_embeds), and the
    text window is then taken exactly as the reference takes it."""

    def __init__(self, keywords, tokenizer, input_ids):
        self.keywords = keywords
        self.keyword_ids = []
        self.max_keyword_len = 0
        for keyword in keywords:
            ids = tokenizer(keyword).input_ids
            if len(ids) > 1 and ids[0] == tokenizer.bos_token_id:
                ids = ids[1:]
            self.max_keyword_len = max(self.max_keyword_len, len(ids))
            self.keyword_ids.append(torch.tensor(ids))
        self.tokenizer = tokenizer
        self.start_len = input_ids.shape[1]

    def call_for_batch(self, output_ids, scores, **kwargs):
        offset = min(output_ids.shape[1] - self.start_len, self.max_keyword_len)
        self.keyword_ids = [k.to(output_ids.device) for k in self.keyword_ids]
        for k in self.keyword_ids:
            # (a row shorter than the keyword cannot end in it: the reference compares the shorter tail by broadcasting or raises)
            if output_ids.shape[1] >= k.shape[0] and (output_ids[0, -k.shape[0]:] == k).all():
                return True
        text = self.tokenizer.batch_decode(output_ids[:, -offset:], skip_special_tokens=True)[0]
        return any(keyword in text for keyword in self.keywords)

    def __call__(self, output_ids, scores, **kwargs):
        return all([self.call_for_batch(output_ids[i].unsqueeze(0), scores) for i in range(output_ids.shape[0])])
