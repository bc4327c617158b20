"""The reference's text baseline on the HIP path: both prompt encoders of a FLUX pipeline directory behind one call.

infer/inference_qwenvl.py:97-119 (get_t5_input_embeds; the other sampling scripts carry the same function) conditions on
  pooled_prompt_embeds = clip_model(clip_ids, output_hidden_states=False).pooler_output     CLIPTextModel, `text_encoder/`, 77 tokens
  prompt_embeds        = t5_model(t5_ids, output_hidden_states=False)[0]                     T5EncoderModel, `text_encoder_2/`
and so does the distillation teacher (train/train_qwenvl.py:665-666, 778-779).  Here the two run as x2i_amd.clip.CLIPTextModel and
x2i_amd.t5.T5EncoderModel.  The entry point takes token ids: no tokenizer vocabulary ships with this repository.  A caller that has the
pipeline's two tokenizer objects passes them in and may then give a `text_prompt` string, tokenized as the reference does it.

Not built: wiring either encoder into the teacher ranks of train_distill.py.
"""
import torch

from .clip import CLIPTextModel
from .t5 import T5EncoderModel


class TextEncoders:
    def __init__(self, clip, t5, clip_tokenizer=None, t5_tokenizer=None):
        self.clip, self.t5 = clip, t5
        self.clip_tokenizer, self.t5_tokenizer = clip_tokenizer, t5_tokenizer

    @classmethod
    def from_pretrained(cls, flux_path, device="cuda", clip_tokenizer=None, t5_tokenizer=None):
        """`text_encoder/` (CLIPTextModel) and `text_encoder_2/` (T5EncoderModel) of a diffusers FLUX pipeline directory"""
        return cls(CLIPTextModel.from_pretrained(flux_path, subfolder="text_encoder", device=device),
                   T5EncoderModel.from_pretrained(flux_path, subfolder="text_encoder_2", device=device), clip_tokenizer, t5_tokenizer)

    @property
    def device(self):
        return self.clip.device

    def tokenize(self, text_prompt):
        """(clip_ids [B, 77], t5_ids [B, S]) of a prompt, with the calls of infer/inference_qwenvl.py:98-116"""
        if self.clip_tokenizer is None or self.t5_tokenizer is None:
            raise ValueError("x2i_amd TextEncoders: a text_prompt needs both tokenizer objects; pass token ids instead")
        kw = dict(return_overflowing_tokens=False, return_length=False, return_tensors="pt")
        return (self.clip_tokenizer(text_prompt, padding="max_length", max_length=77, truncation=True, **kw).input_ids,
                self.t5_tokenizer(text_prompt, **kw).input_ids)

    @torch.no_grad()
    def get_t5_input_embeds(self, clip_ids=None, t5_ids=None, text_prompt=None):
        """-> (pooled_prompt_embeds bf16 [B, hidden of CLIP], prompt_embeds bf16 [B, S, d_model of T5]) on the encoders' device"""
        if text_prompt is not None:
            if clip_ids is not None or t5_ids is not None:
                raise ValueError("x2i_amd TextEncoders: pass either token ids or a text_prompt")
            clip_ids, t5_ids = self.tokenize(text_prompt)
        if clip_ids is None or t5_ids is None:
            raise ValueError("x2i_amd TextEncoders: both clip_ids and t5_ids are needed")
        pooled = self.clip(clip_ids.to(self.device), output_hidden_states=False).pooler_output
        embeds = self.t5(t5_ids.to(self.device), output_hidden_states=False)[0]
        return pooled, embeds
