#!/usr/bin/env python3
"""Qwen2.5-VL (3B / 7B) -> X2I sampling on the HIP path.  Counterpart of infer/inference_qwenvl.py.

  python -m x2i_amd.infer.inference_qwenvl --qwen_size 7b --flux_path <dir> --proj_path <bin> --task text2image
  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m x2i_amd.infer.inference_qwenvl --batch 32 ...
  python -m x2i_amd.infer.inference_qwenvl --synthetic --task text2image        # no checkpoints needed
"""
import torch

from .harness import Harness, SyntheticConditioner, asset, build_parser, sample_seed, stack_hidden_states


class QwenVLConditioner:
    """Qwen2_5_VLForConditionalGeneration prompt pass; inputs padded to 512 tokens, images resized to 128x128, videos at
    1 fps / 128*128 pixels, generate(max_new_tokens=128, output_hidden_states=True) -- infer/inference_qwenvl.py:136-180."""

    def __init__(self, path, device, use_answer=False, prefill_only=True, hip_decoder=False, hip_vision=False, hip_generate=False, hip_head=False,
                 hip_w8=False, hip_sample=False, hip_sample_seed=0, hip_image=False, model=None, processor=None):
        if hip_w8 and not hip_generate:         # (before the checkpoint is read)
            raise ValueError("--hip_w8 runs the decode steps of --hip_generate's loop on e4m3 weights: not without --hip_generate")
        if hip_sample and not (hip_generate and hip_head):
            raise ValueError("--hip_sample draws the tokens inside --hip_generate --hip_head's captured step: not without both")
        if model is None or processor is None:  # model / processor: hand in loaded ones (a test's stand-ins) and `path` is not read
            from transformers import AutoProcessor, Qwen2_5_VLForConditionalGeneration
            model = model if model is not None else Qwen2_5_VLForConditionalGeneration.from_pretrained(path, torch_dtype=torch.bfloat16).eval().to(device)
            processor = processor if processor is not None else AutoProcessor.from_pretrained(path)
        self.model, self.processor = model, processor
        self.device, self.use_answer = device, use_answer
        # the prompt-pass states are all the reference keeps unless --use_answer: take them from ONE forward, written by
        # hooks straight into the [B,C,S,H] buffer (x2i_amd/handoff.py), instead of a 128-token generate() + torch.cat
        self.slab = None
        if hip_decoder and not (prefill_only and not use_answer):
            raise ValueError("--hip_decoder serves the prompt pass only: not with --full_generate or --use_answer")
        # hip_generate: the whole greedy generate() with the decoder stack on the HIP path (handoff.HipGenerate): the generated tokens' states
        # under --use_answer, the prompt's otherwise
        self.generate = None
        if hip_head and not hip_generate:
            raise ValueError("--hip_head chooses the tokens of --hip_generate's loop: not without --hip_generate")
        if hip_generate:
            if hip_decoder:
                raise ValueError("--hip_generate runs the prompt pass on the HIP path itself: not together with --hip_decoder")
            from ..handoff import HipGenerate
            if not hip_sample:
                HipGenerate.refuse_sampling(self.model.generation_config)
            self.generate = HipGenerate(self.model, hip_head=hip_head, w8=hip_w8, sample=hip_sample, seed=hip_sample_seed)
        elif prefill_only and not use_answer:
            from ..handoff import HiddenStateSlab, HipPrefill, find_decoder
            # hip_decoder: the same one forward with the decoder stack itself on the HIP path (x2i_amd/qwen.py)
            self.slab = HipPrefill(self.model) if hip_decoder else HiddenStateSlab(find_decoder(self.model))

        # hip_vision: the vision tower behind model.visual on the HIP path (x2i_amd/qwen_vision.py), under either kind of slab and under
        # generate() alike: the surrounding model still calls it through get_image_features / get_video_features
        self.vision = None
        if hip_vision:
            from ..handoff import HipVision
            self.vision = HipVision(self.model).install()

        # hip_image: the tower's input on the HIP path (x2i_amd/qwen_image.py) in place of the processor's Qwen2VLImageProcessor: smart_resize,
        # Pillow's BICUBIC resize, the normalisation and the patch rows [S, 1176] in one launch per run of equally sized images, bit for bit
        # the processor's values.  The reference's own 128 x 128 resize stays on the host in front of it (49 KB to upload per image).  With
        # hip_vision the rows are written as bf16 straight into the tower's padded workspace, which HipVision then does not copy.
        self.image = None
        if hip_image:
            from ..handoff import HipQwenImage
            self.image = HipQwenImage(self.processor, device, tower=self.vision.tower if self.vision is not None else None).install()

    @torch.no_grad()
    def __call__(self, videos=None, images=None, audios=None, text_prompt=None):
        from PIL import Image
        content, image_list, video_inputs = [], [], None
        for path in images or []:
            im = Image.open(path).convert("RGB").resize(size=(128, 128))
            content.append({"type": "image", "image": im})
            image_list.append(im)
        if videos:
            assert len(videos) == 1
            from qwen_vl_utils import process_vision_info
            content.append({"type": "video", "video": videos[0], "max_pixels": 128 * 128, "fps": 1.0})
            _, video_inputs = process_vision_info([{"role": "user", "content": content}])
        if text_prompt is not None:
            content.append({"type": "text", "text": text_prompt})
        message = [{"role": "user", "content": content}]
        prompt = self.processor.apply_chat_template(message, tokenize=False, add_generation_prompt=True)
        inputs = self.processor(text=[prompt], images=image_list or None, videos=video_inputs, padding="max_length",
                                max_length=512, truncation=True, return_tensors="pt").to(self.device)
        if self.generate is not None:
            gc = self.model.generation_config
            out = self.generate.generate(self.model, max_new_tokens=128, eos_token_id=gc.eos_token_id, pad_token_id=gc.pad_token_id,
                                         logits_processor=self.model._get_logits_processor(gc, input_ids_seq_length=inputs["input_ids"].shape[1],
                                                                                               device=self.device), **inputs)
            return out.answer if self.use_answer else out.prompt
        if self.slab is not None:
            return self.slab.prefill(self.model, **inputs)
        out = self.model.generate(**inputs, max_new_tokens=128, output_hidden_states=True, return_dict_in_generate=True)
        return stack_hidden_states(out["hidden_states"], use_answer=self.use_answer)


def tasks(args):
    img = lambda n: asset(args, "image", n)
    vid = lambda n: asset(args, "video", n)
    return {
        "text2image": [dict(filename="elephant_%s" % k, text_prompt=p) for k, p in (
            ("EN", "A majestic elephant in a sun-drenched savannah, impressionistic style, low camera angle."),
            ("ZH", "一只雄伟的大象站在阳光普照的草原上，印象派风格，低机位。"),
            ("DE", "Ein majestätischer Elefant in einer sonnenüberfluteten Savanne, impressionistischer Stil."),
            ("FR", "Un éléphant majestueux dans une savane baignée de soleil, style impressionniste."),
            ("JA", "日差しに照らされたサバンナに立つ荘厳な象、印象派のスタイル。"),
            ("VI", "Một con voi uy nghi trên thảo nguyên đầy nắng, phong cách ấn tượng."))],
        "image2image": [dict(filename="sea_moon", images=[img("sea_moon.jpg")]),
                        dict(filename="dog_hat", images=[img("dog.jpg"), img("hat.jpg")])],
        "imagetext2image": [dict(filename="yarn_ball_panda", images=[img("yarn_ball.jpg")],
                                 text_prompt="Refer to the image style and generate a cute giant panda"),
                            dict(filename="hutong_car", images=[img("hutong.jpg")], text_prompt="Add a car in the picture")],
        "video2image": [dict(filename="particle_collision", videos=[vid("particle_collision.mp4")]),
                        dict(filename="Skiing", videos=[vid("Skiing.mp4")])],
        "x2image": [dict(filename="Shuimohua", images=[img("Shuimohua.jpg")]),
                    dict(filename="particle_collision_x", videos=[vid("particle_collision.mp4")])],
    }


def main(argv=None):
    args = build_parser("qwenvl").parse_args(argv)
    kind = "qwen" + args.qwen_size
    device = "cuda:%d" % int(__import__("os").environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(device)
    cond = SyntheticConditioner(kind, device) if args.synthetic else QwenVLConditioner(args.qwen_path, device, args.use_answer, prefill_only=not args.full_generate,
                                                                                            hip_decoder=args.hip_decoder, hip_vision=args.hip_vision,
                                                                                            hip_generate=args.hip_generate, hip_head=args.hip_head,
                                                                                            hip_w8=args.hip_w8, hip_sample=args.hip_sample,
                                                                                            hip_sample_seed=sample_seed(args), hip_image=args.hip_image)
    Harness(args, kind, cond, device).run_tasks(tasks(args))


if __name__ == "__main__":
    main()
