"""tokenizer_image_token of the reference (llava/mm_utils.py:43-62): tokenise the text around each `<image>` tag and
put IMAGE_TOKEN_INDEX between the pieces, keeping a single leading BOS."""
import torch

from llava.constants import IMAGE_TOKEN_INDEX


def tokenizer_image_token(prompt, tokenizer, image_token_index=IMAGE_TOKEN_INDEX, return_tensors=None):
    pieces = [tokenizer(part).input_ids for part in prompt.split("<image>")]
    lead_bos = bool(pieces) and bool(pieces[0]) and pieces[0][0] == tokenizer.bos_token_id
    skip = 1 if lead_bos else 0
    ids = [pieces[0][0]] if lead_bos else []
    for n, piece in enumerate(pieces):
        if n > 0:
            ids.append(image_token_index)
        ids.extend(piece[skip:])
    if return_tensors is None:
        return ids
    if return_tensors == "pt":
        return torch.tensor(ids, dtype=torch.long)
    raise ValueError(f"Unsupported tensor type: {return_tensors}")


def _pad_to_square(img, fill):
    """PIL image -> square canvas of the longer side filled with `fill`, the image centred (the trainer's `pad` aspect rule,
    llava/train/train_halva.py:_expand2square)."""
    from PIL import Image
    w, h = img.size
    if w == h:
        return img
    side = max(w, h)
    canvas = Image.new(img.mode, (side, side), fill)
    canvas.paste(img, ((side - w) // 2, (side - h) // 2))
    return canvas


def process_images(images, image_processor, model_cfg):
    """PIL images -> pixel values [N, 3, S, S] as the trainer preprocesses them (llava/train/train_halva.py:_load_image): with
    image_aspect_ratio == "pad" each image is padded to a square in the processor's mean colour first, then CLIP-preprocessed.
    A list is returned when the results differ in shape."""
    if getattr(model_cfg, "image_aspect_ratio", None) != "pad":
        return image_processor(images, return_tensors="pt")["pixel_values"]
    fill = tuple(int(x * 255) for x in image_processor.image_mean)
    out = [image_processor.preprocess(_pad_to_square(im, fill), return_tensors="pt")["pixel_values"][0] for im in images]
    return torch.stack(out, 0) if all(x.shape == out[0].shape for x in out) else out


def get_model_name_from_path(model_path):
    """Last path component, or `<run>_checkpoint-<n>` for a checkpoint directory inside a run."""
    parts = model_path.strip("/").split("/")
    return parts[-2] + "_" + parts[-1] if parts[-1].startswith("checkpoint-") and len(parts) > 1 else parts[-1]
