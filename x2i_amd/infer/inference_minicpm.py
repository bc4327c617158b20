#!/usr/bin/env python3
"""MiniCPM-o-2.6 (image / video / audio / text) -> X2I sampling on the HIP path.  Counterpart of infer/inference_minicpm.py:
unpadded inputs, generate(max_new_tokens=1, decode_text=False), torch.stack(hidden_states[0], dim=1) (:116-118,160-177)."""
import torch

from .harness import Harness, SyntheticConditioner, asset, build_parser, stack_hidden_states

MAX_NUM_FRAMES = 64


def encode_video(path):
    """1 frame per second, uniformly thinned to MAX_NUM_FRAMES (inference_minicpm.py:120-135)."""
    from decord import VideoReader, cpu
    from PIL import Image
    vr = VideoReader(path, ctx=cpu(0))
    idx = list(range(0, len(vr), max(1, round(vr.get_avg_fps()))))
    if len(idx) > MAX_NUM_FRAMES:
        gap = len(idx) / MAX_NUM_FRAMES
        idx = [idx[int(i * gap + gap / 2)] for i in range(MAX_NUM_FRAMES)]
    return [Image.fromarray(f.astype("uint8")) for f in vr.get_batch(idx).asnumpy()]


class MiniCPMConditioner:
    """prefill_only (default): the [1, C, S, H] conditioning tensor is written by hooks on the LLM decoder during the ONE prompt
    pass of generate(max_new_tokens=1) (x2i_amd/handoff.py, row N2) -- no hidden-state tuple, no torch.stack copy, and no
    dependence on the reference's patched generate() returning `.hidden_states`.  full_generate: the reference's form."""

    def __init__(self, path, device, prefill_only=True, model=None, tokenizer=None, processor=None, hip_vision=False, hip_resampler=False,
                 hip_audio=False, hip_decoder=False, use_answer=False, hip_mel=False, hip_image=False, max_slice_nums=1):
        if hip_decoder and not (prefill_only and not use_answer):     # (refused before a checkpoint is read)
            raise ValueError("--hip_decoder serves the prompt pass only: not with --full_generate or --use_answer")
        if model is None:
            from transformers import AutoModel, AutoProcessor, AutoTokenizer
            model = AutoModel.from_pretrained(path, trust_remote_code=True, torch_dtype=torch.bfloat16).eval().to(device)
            tokenizer = AutoTokenizer.from_pretrained(path, trust_remote_code=True)
            processor = AutoProcessor.from_pretrained(path, trust_remote_code=True)
        self.model, self.tokenizer, self.processor = model, tokenizer, processor
        self.device = device
        self.slab = self.prompt = None
        if hip_decoder:
            # hip_decoder: the embedding merge and the decoder stack of the prompt pass on the HIP path (handoff.HipMiniCPMPrompt): the towers
            # below -- the model's own or their HIP forms -- feed ONE merge launch that writes layer 0's input, and no lm_head runs
            from ..handoff import HipMiniCPMPrompt
            self.prompt = HipMiniCPMPrompt(self.model)
        elif prefill_only:
            from ..handoff import HiddenStateSlab, find_decoder
            self.slab = HiddenStateSlab(find_decoder(self.model))
        # hip_vision: the SigLIP tower behind model.vpm on the HIP path (x2i_amd/siglip.py), under the slab and under the reference's
        # generate() alike: get_vllm_embedding still calls it, and the embedding scatter stays the model's own
        self.vision = None
        if hip_vision:
            from ..handoff import HipSiglip
            self.vision = HipSiglip(self.model).install()
        # hip_resampler: the perceiver behind model.resampler on the HIP path (x2i_amd/resampler.py); without it the Resampler stays the
        # model's own, with or without hip_vision
        self.resampler = None
        if hip_resampler:
            from ..handoff import HipResampler
            self.resampler = HipResampler(self.model).install()
        # hip_audio: the Whisper tower, the projector and the pooling behind get_audio_embedding on the HIP path (x2i_amd/whisper.py), under
        # either kind of slab; the embedding scatter stays the model's own
        self.audio = None
        if hip_audio:
            from ..handoff import HipAudio
            self.audio = HipAudio(self.model).install()
        # hip_mel: the log-mel features of an audio prompt on the HIP path (x2i_amd/logmel.py) in place of the processor's feature extractor:
        # the processor hands on device tensors, and with hip_audio the tower reads them where they are
        self.mel = None
        if hip_mel:
            from ..handoff import HipLogMel
            self.mel = HipLogMel(self.processor, device).install()
        # hip_image: the pixel_values of images that are not sliced (a video's frames) on the HIP path (x2i_amd/image.py) in place of the
        # processor's image processor: the processor hands on device tensors, bit for bit the host's values
        # max_slice_nums: what the processor is called with (1, the reference's value: no image is sliced).  Above 1 the hand-off serves
        # the sliced images too: the source image and the crops of the slicing grid (include/frontend/tiles/x2i_image_tiles.h)
        self.max_slice_nums = int(max_slice_nums)
        if self.max_slice_nums < 1:
            raise ValueError("--max_slice_nums must be at least 1 (got %d)" % self.max_slice_nums)
        self.image = None
        if hip_image:
            from ..handoff import HipImage
            self.image = HipImage(self.processor, device, slices=self.max_slice_nums > 1).install()

    def hidden_states(self, inputs):
        """processor outputs -> [B, C, S, H]"""
        if self.prompt is not None:
            return self.prompt.prompt(**inputs)
        run = lambda: self.model.generate(**inputs, tokenizer=self.tokenizer, max_new_tokens=1, decode_text=False)  # noqa: E731
        if self.slab is not None:
            return self.slab.capture(run)
        return stack_hidden_states(run().hidden_states)

    @torch.no_grad()
    def __call__(self, videos=None, images=None, audios=None, text_prompt=None):
        from PIL import Image
        text, image_list, audio_list = "", [], []
        for p in images or []:
            image_list.append(Image.open(p).convert("RGB"))
            text += "(<image>./</image>)\n"
        for v in videos or []:
            frames = encode_video(v)
            text += "(<image>./</image>)\n" * len(frames)
            image_list.extend(frames)
        for a in audios or []:
            import librosa
            wav, _ = librosa.load(a, sr=16000, mono=True)
            text += "(<audio>./</audio>)\n"
            audio_list.append(wav)
        text += text_prompt or ""
        prompt = self.processor.tokenizer.apply_chat_template([{"role": "user", "content": text}], tokenize=False,
                                                              add_generation_prompt=True)
        inputs = self.processor(text=[prompt], images=[image_list] if image_list else None,
                                audios=[audio_list] if audio_list else None, max_slice_nums=self.max_slice_nums, use_image_id=False,
                                chunk_input=True, return_tensors="pt", max_length=32768, sampling_rate=16000,
                                add_special_tokens=True).to(self.device)
        inputs.pop("image_sizes")
        return self.hidden_states(inputs)


def tasks(args):
    img = lambda n: asset(args, "image", n)
    return {
        "text2image": [dict(filename="elephant", text_prompt="A majestic elephant in a sun-drenched savannah.")],
        "image2image": [dict(filename="sea_moon", images=[img("sea_moon.jpg")])],
        "imagetext2image": [dict(filename="man_smile", images=[img("man.jpg")], text_prompt="Make the person in the picture smile")],
        "video2image": [dict(filename="Skiing", videos=[asset(args, "video", "Skiing.mp4")])],
        "audio2image": [dict(filename="audio", audios=[asset(args, "audio", "thunder.wav")])],
    }


def main(argv=None):
    args = build_parser("minicpm").parse_args(argv)
    device = "cuda:%d" % int(__import__("os").environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(device)
    cond = SyntheticConditioner("minicpm", device) if args.synthetic else MiniCPMConditioner(args.minicpm_path, device,
                                                                                              prefill_only=not args.full_generate,
                                                                                              hip_vision=args.hip_vision,
                                                                                              hip_resampler=args.hip_resampler,
                                                                                              hip_audio=args.hip_audio,
                                                                                              hip_mel=args.hip_mel,
                                                                                              hip_image=args.hip_image,
                                                                                              max_slice_nums=args.max_slice_nums,
                                                                                              hip_decoder=args.hip_decoder,
                                                                                              use_answer=args.use_answer)
    Harness(args, "minicpm", cond, device).run_tasks(tasks(args))


if __name__ == "__main__":
    main()
