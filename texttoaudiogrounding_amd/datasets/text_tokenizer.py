"""DictTokenizer (mirror of datasets/text_tokenizer.py:9-58 in the reference): whitespace-split phrases -> vocabulary ids,
zero-padded to the longest phrase; ``List[str]`` -> text (B,L) / text_len (B,); ``List[List[str]]`` (the same number of
phrases per clip) -> text (B,N,L) / text_len (B,N).  int64 tensors, pad id 0 (= ``<pad>``).
HuggingFaceTokenizer (mirror of datasets/text_tokenizer.py:61-96): a locally available ``AutoTokenizer`` -> input_ids /
attention_mask / text_len of the same two shapes."""
import pickle
from typing import List, Union

import torch

from ..utils.build_vocab import Vocabulary


class DictTokenizer:
    def __init__(self, vocabulary) -> None:
        self.vocabulary = Vocabulary()
        if isinstance(vocabulary, dict):
            self.vocabulary.load_state_dict(vocabulary)
        else:
            with open(vocabulary, "rb") as f:
                self.vocabulary.load_state_dict(pickle.load(f))

    def _encode(self, phrases: List[str]):
        ids = [[self.vocabulary(tok) for tok in p.split()] for p in phrases]
        lens = torch.tensor([len(x) for x in ids], dtype=torch.long)
        text = torch.zeros(len(ids), int(lens.max()) if len(ids) else 0, dtype=torch.long)
        for row, x in zip(text, ids):
            row[:len(x)] = torch.tensor(x, dtype=torch.long)
        return text, lens

    def __call__(self, texts: Union[List[str], List[List[str]]]):
        assert isinstance(texts, list), "the input must be List[str] or List[List[str]]"
        if isinstance(texts[0], str):
            text, lens = self._encode(texts)
        elif isinstance(texts[0], list):
            n = len(texts[0])
            assert all(len(t) == n for t in texts), "the text number in each list must be the same"
            text, lens = self._encode([p for t in texts for p in t])
            text, lens = text.reshape(len(texts), n, -1), lens.reshape(len(texts), n)
        else:
            raise TypeError("the input must be List[str] or List[List[str]]")
        return {"text": text, "text_len": lens}

    def inverse_transform(self, texts):
        out = []
        for row in texts:
            words = []
            for idx in row:
                idx = int(idx)
                if idx == 0:
                    break
                words.append(self.vocabulary.idx2word[idx])
            out.append(" ".join(words))
        return out


class HuggingFaceTokenizer:
    """datasets/text_tokenizer.py:61-96: ``AutoTokenizer`` of ``model_name`` (default ``laion/clap-htsat-fused``), padded to the
    longest phrase and truncated: ``List[str]`` -> ``input_ids`` / ``attention_mask`` (B, L) and ``text_len`` (B,) = the mask's
    row sums; ``List[List[str]]`` (the same number of phrases per clip) -> (B, N, L) / (B, N).  int64 tensors -- what
    ``models.text_encoder.LaionClapEncoder`` reads.

    The tokenizer is loaded with ``local_files_only=True``: ``model_name`` must be a directory written by
    ``tokenizer.save_pretrained`` or a name already in the Hugging Face cache; the network is never touched and a name that does
    not resolve raises a RuntimeError that says so."""

    def __init__(self, model_name: str = "laion/clap-htsat-fused") -> None:
        try:
            from transformers import AutoTokenizer
            self.core = AutoTokenizer.from_pretrained(model_name, local_files_only=True)
        except Exception as e:                              # noqa: BLE001 - not cached / no such directory / no transformers
            raise RuntimeError(
                f"HuggingFaceTokenizer: the tokenizer {model_name!r} is not available locally ({type(e).__name__}); it is loaded "
                "with local_files_only=True and never downloaded. Pass a directory written by tokenizer.save_pretrained(...) or "
                "fill the Hugging Face cache beforehand") from e

    def __call__(self, texts: Union[List[str], List[List[str]]]):
        assert isinstance(texts, list), "the input must be List[str] or List[List[str]]"
        if isinstance(texts[0], str):
            out = dict(self.core(texts, padding=True, return_tensors="pt", truncation=True))
        elif isinstance(texts[0], list):
            n = len(texts[0])
            assert all(len(t) == n for t in texts), "the text number in each list must be the same"
            flat = self.core([p for t in texts for p in t], padding=True, return_tensors="pt", truncation=True)
            out = {k: v.reshape(len(texts), n, *v.shape[1:]) for k, v in flat.items()}
        else:
            raise TypeError("the input must be List[str] or List[List[str]]")
        out["text_len"] = out["attention_mask"].sum(dim=-1)
        return out
