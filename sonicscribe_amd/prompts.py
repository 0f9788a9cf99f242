"""ASRModel's `.prompt`, from a request to its prompt ids and from token ids to text: the checkpoint's tokenizer + chat template, or the stand-in without one."""
from __future__ import annotations

from typing import Any, Dict, List, Sequence

from . import frontend
from .spec import ModelDims


class SyntheticPrompt:
    """Stand-in for the checkpoint's tokenizer + chat template (absent offline): fixed prefix / suffix ids
    around the audio placeholders.  Decoding renders ids as text so the call surface stays str-valued."""

    def __init__(self, dims: ModelDims, prefix: Sequence[int] = (1, 17, 23, 5), suffix: Sequence[int] = (7, 301, 302, 303, 9, 11)):
        self.dims, self.prefix, self.suffix = dims, list(prefix), list(suffix)

    def build(self, instruction: str, n_audio: int) -> List[int]:
        extra = [] if instruction == frontend.BASE_INSTRUCTION else [2 + (sum(instruction.encode()) % 200)]
        return self.prefix + [self.dims.audio_token_id] * n_audio + self.suffix + extra

    def decode(self, ids: Sequence[int]) -> str:
        eos = set(self.dims.eos_ids)
        return " ".join(str(int(i)) for i in ids if int(i) not in eos)


class HFPrompt:
    """Tokenizer + chat template of a real checkpoint (processing_glmasr.py:178-180: the audio placeholder string is
    repeated ``num_audio_tokens`` times before tokenisation).  Prompts are cached per (instruction, n_audio) -- SURVEY §8f4."""

    def __init__(self, processor, dims: ModelDims):
        self.processor, self.dims = processor, dims
        self.audio_token = getattr(processor, "audio_token", "<|pad|>")
        self._cache: Dict[Any, List[int]] = {}

    def build(self, instruction: str, n_audio: int) -> List[int]:
        key = (instruction, n_audio)
        if key not in self._cache:
            messages = [{"role": "user", "content": [{"type": "audio", "url": ""}, {"type": "text", "text": instruction}]}]
            text = self.processor.tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True,
                                                                chat_template=self.processor.chat_template)
            text = text.replace(self.audio_token, self.audio_token * n_audio, 1)
            self._cache[key] = list(self.processor.tokenizer(text, add_special_tokens=False)["input_ids"])
        return self._cache[key]

    def decode(self, ids: Sequence[int]) -> str:
        return self.processor.batch_decode([list(map(int, ids))], skip_special_tokens=True)[0]
