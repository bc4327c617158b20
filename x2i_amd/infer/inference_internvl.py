#!/usr/bin/env python3
"""InternVL2.5 (1B / 4B) -> X2I sampling on the HIP path.  Counterpart of infer/inference_internvl.py: tokens padded to
512 (:126), the (locally modified) chat model's generate() is ONE forward that returns every layer's hidden states
(model_internvl/internvl/modeling_internvl_chat.py:314-363), default seed 1 (:192), tasks text2image / image2image /
imagetext2image only (:288-294)."""
import torch

from .harness import Harness, SyntheticConditioner, asset, build_parser

# the constants of the reference's prompt (infer/inference_internvl.py:94-131, the `internvl2_5` conversation template)
IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN = "<img>", "</img>", "<IMG_CONTEXT>"
NUM_IMAGE_TOKEN = 256
SYSTEM_MESSAGE = "你是书生·万象，英文名是InternVL，是由上海人工智能实验室、清华大学及多家合作单位联合开发的多模态大语言模型。"
SYSTEM_TEMPLATE = "<|im_start|>system\n{system_message}"
ROLES = ("<|im_start|>user\n", "<|im_start|>assistant\n")
SEP = "<|im_end|>\n"


def build_query(text_prompt, num_patches_list=(), num_image_token=NUM_IMAGE_TOKEN, system_message=SYSTEM_MESSAGE, roles=ROLES, sep=SEP):
    """The string the reference tokenises (its gene_token, infer/inference_internvl.py:94-131,165-176): the text wrapped as
    str({"Text input": ..., "Instruction editing description": "no"}), `<image>\n` in front once per entry of num_patches_list (the
    reference takes one image), that question as the user turn of the `internvl2_5` template with an open assistant turn, and every
    `<image>` replaced by <img> + num_image_token * tiles context tokens + </img>: the rows the vision features are merged into.
    A pure function of its arguments."""
    question = str({"Text input": text_prompt, "Instruction editing description": "no"})
    if num_patches_list and "<image>" not in question:
        question = "<image>\n" * len(num_patches_list) + question
    query = SYSTEM_TEMPLATE.format(system_message=system_message) + sep + roles[0] + question + sep + roles[1]
    for tiles in num_patches_list:
        query = query.replace("<image>", IMG_START_TOKEN + IMG_CONTEXT_TOKEN * num_image_token * tiles + IMG_END_TOKEN, 1)
    return query


class InternVLConditioner:
    """prefill_only (default): hooks on the language model's decoder stack fill the [1, C, 512, H] tensor during the first
    decoder pass of the chat model's generate() (x2i_amd/handoff.py, row N2).  That works with the STOCK InternVL2.5 remote code
    (whose generate() returns token ids); full_generate expects the reference's locally modified modeling_internvl_chat.py, whose
    generate() is one forward returning every layer's hidden states (model_internvl/internvl/modeling_internvl_chat.py:314-363)."""

    def __init__(self, path, device, prefill_only=True, model=None, tokenizer=None, hip_vision=False, hip_decoder=False, use_answer=False,
                 hip_image=False):
        if hip_decoder and not (prefill_only and not use_answer):     # (refused before a checkpoint is read)
            raise ValueError("--hip_decoder serves the prompt pass only: not with --full_generate or --use_answer")
        if model is None:
            from transformers import AutoModel, AutoTokenizer
            model = AutoModel.from_pretrained(path, trust_remote_code=True, torch_dtype=torch.bfloat16).eval().to(device)
            tokenizer = AutoTokenizer.from_pretrained(path, trust_remote_code=True, use_fast=False)
        self.model, self.tokenizer = model, tokenizer
        self.device = device
        self.slab = self.prompt = None
        if hip_decoder:
            # hip_decoder: the embedding merge and the decoder stack of the prompt pass on the HIP path (handoff.HipInternVLPrompt):
            # extract_feature -- the model's own or hip_vision's -- feeds ONE merge launch that writes layer 0's input; no lm_head runs
            from ..handoff import HipInternVLPrompt
            self.prompt = HipInternVLPrompt(self.model)
        elif prefill_only:
            from ..handoff import HiddenStateSlab, find_decoder
            self.slab = HiddenStateSlab(find_decoder(self.model))
        # hip_vision: what extract_feature computes (vision_model, pixel_shuffle, mlp1) on the HIP path (x2i_amd/internvit.py), under the
        # slab and under the reference's generate() alike: the chat model still calls extract_feature, and the scatter stays its own
        self.vision = None
        if hip_vision:
            from ..handoff import HipInternVision
            self.vision = HipInternVision(self.model).install()
        # hip_image: the 448 x 448 tile of an image on the HIP path (x2i_amd/internvl_image.py): the 128 x 128 shrink stays on the host, its
        # resize to the tile and the normalisation run on the device, bit for bit the tile computed below without the flag
        self.image = None
        if hip_image:
            from ..internvl_image import InternVLImageFrontEnd
            self.image = InternVLImageFrontEnd(448, device=device)

    def hidden_states(self, pixel_values, input_ids, attention_mask):
        if self.prompt is not None:
            return self.prompt.prompt(input_ids, attention_mask, pixel_values)
        if self.slab is not None:
            return self.slab.capture(lambda: self.model.generate(pixel_values=pixel_values, input_ids=input_ids,
                                                                 attention_mask=attention_mask, max_new_tokens=1))
        hs = self.model.generate(pixel_values=pixel_values, input_ids=input_ids, attention_mask=attention_mask)
        return torch.stack(tuple(hs), dim=1)

    def image_tiles(self, images):
        """bf16 [images, 3, 448, 448] on the device: per image a 128 x 128 resize, then a single 448 x 448 ImageNet-normalised tile
        (inference_internvl.py:171)"""
        from PIL import Image
        import numpy as np
        small = [Image.open(p).convert("RGB").resize((128, 128)) for p in images]
        if self.image is not None:      # max_num = 1: one tile per image; bf16 as one rounding of the float32 value, like .to(bfloat16) below
            return self.image.tiles(small, max_num=1, out_dtype=torch.bfloat16)[0]
        tiles = []
        for im in small:
            a = torch.from_numpy(np.asarray(im.resize((448, 448)))).float().div(255).permute(2, 0, 1)
            mean, std = torch.tensor([0.485, 0.456, 0.406])[:, None, None], torch.tensor([0.229, 0.224, 0.225])[:, None, None]
            tiles.append((a - mean) / std)
        return torch.stack(tiles).to(self.device, torch.bfloat16)

    @torch.no_grad()
    def __call__(self, videos=None, images=None, audios=None, text_prompt=None):
        pixel_values = self.image_tiles(images) if images else None
        # one 448 x 448 tile per image; the context tokens the features are merged into come with the query (as the chat model's own chat()
        # does, the id of the context token is set on the model before generate() looks for it)
        q = build_query(text_prompt, [1] * len(images or []), getattr(self.model, "num_image_token", NUM_IMAGE_TOKEN))
        self.model.img_context_token_id = self.tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        tok = self.tokenizer(q, padding="max_length", max_length=512, truncation=True, return_tensors="pt").to(self.device)
        return self.hidden_states(pixel_values, tok.input_ids, tok.attention_mask)


def tasks(args):
    img = lambda n: asset(args, "image", n)
    return {
        "text2image": [dict(filename="elephant", text_prompt="A majestic elephant in a sun-drenched savannah.")],
        "image2image": [dict(filename="sea_moon", images=[img("sea_moon.jpg")])],
        "imagetext2image": [dict(filename="hutong_car", images=[img("hutong.jpg")], text_prompt="Add a car in the picture")],
    }


def main(argv=None):
    p = build_parser("internvl")
    p.set_defaults(seed=1)
    args = p.parse_args(argv)
    kind = "internvl" + args.internvl_size
    device = "cuda:%d" % int(__import__("os").environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(device)
    cond = SyntheticConditioner(kind, device) if args.synthetic else InternVLConditioner(args.internvl_path, device,
                                                                                         prefill_only=not args.full_generate,
                                                                                         hip_vision=args.hip_vision, hip_decoder=args.hip_decoder,
                                                                                         use_answer=args.use_answer, hip_image=args.hip_image)
    Harness(args, kind, cond, device).run_tasks(tasks(args))


if __name__ == "__main__":
    main()
