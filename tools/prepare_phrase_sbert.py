#!/usr/bin/env python3
"""Phrase / label embeddings from a sentence-transformers BERT model, as the ``{text: float32 vector}`` pickles that
tools/map_phrase_to_event.py, tools/kmeans_emb.py and the other clustering tools read.  The reference's
utils/data/create_text_embedding/prepare_phrase_sbert.py runs ``SentenceTransformer(model_type).encode``; here
``models.text_encoder.SentenceBert`` reads the same LOCAL model directory and runs on the HIP text tower through
``utils.text_embed.PhraseEmbedder`` (phrases sorted by token count, batches padded to their own longest phrase; truncation at
min(max_seq_length, 64) tokens).  The ``sentence_transformers`` package is not needed; parity with it is unpinned.  No fallback.

    python tools/prepare_phrase_sbert.py phrase --input label.json --output phrase_emb.pkl --model_type DIR [--debug]
    python tools/prepare_phrase_sbert.py check_add_missing --label label.json --phrase_emb phrase_emb.pkl --model_type DIR
    python tools/prepare_phrase_sbert.py label --input label_encoder.pkl --output label_emb.pkl --model_type DIR
"""
import argparse
import json
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = parser.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("--model_type", type=str, default="all-MiniLM-L6-v2", help="a LOCAL sentence-transformers directory")
        p.add_argument("--device", type=str, default="cuda:0")
        p.add_argument("--batch_tokens", type=int, default=16384, help="largest batch, in padded tokens")
    p = sub.add_parser("phrase", help="the unique phrases of a label JSON -> pickle")
    p.add_argument("--input", type=str, required=True, help="label JSON: [{..., 'phrases': [{'phrase': str, ...}]}]")
    p.add_argument("--output", type=str, required=True)
    p.add_argument("--debug", action="store_true", help="the first 51 clips only")
    common(p)
    p = sub.add_parser("check_add_missing", help="add the phrases of a label JSON that a pickle lacks (in place)")
    p.add_argument("--label", type=str, required=True)
    p.add_argument("--phrase_emb", type=str, required=True)
    common(p)
    p = sub.add_parser("label", help="the classes of a pickled LabelEncoder -> pickle")
    p.add_argument("--input", type=str, required=True)
    p.add_argument("--output", type=str, required=True)
    common(p)
    return parser


def collect_phrases(data, debug=False, skip=()):
    """The unique phrases of a label JSON in first-seen order (the reference's ``list(set(...))`` has no order to keep)."""
    seen = {}
    for idx, audio_item in enumerate(data):
        for item in audio_item["phrases"]:
            phrase = item["phrase"] if isinstance(item, dict) else item
            if phrase not in skip:
                seen.setdefault(phrase, None)
        if debug and idx >= 50:
            break
    return list(seen)


def load_embedder(args):
    from texttoaudiogrounding_amd.models.text_encoder import SentenceBert
    from texttoaudiogrounding_amd.utils.text_embed import PhraseEmbedder
    from transformers import AutoTokenizer
    if not os.path.isdir(args.model_type):
        raise SystemExit(f"{args.model_type}: not a local sentence-transformers directory (the network is never touched)")
    enc = SentenceBert(args.model_type).to(args.device).eval()
    tok = AutoTokenizer.from_pretrained(enc._tokenizer_dir, local_files_only=True)
    return PhraseEmbedder(enc, tok, batch_tokens=args.batch_tokens, max_length=min(enc.max_seq_length, enc.MAX_TOKENS))


def embed_into(table, texts, embedder):
    texts = list(texts)
    if texts:
        for text, emb in zip(texts, embedder.encode(texts)):
            table[text] = emb
    return table


def main(args, embedder=None):
    embedder = embedder or load_embedder(args)
    if args.command == "phrase":
        with open(args.input) as f:
            phrases = collect_phrases(json.load(f), args.debug)
        table, output = embed_into({}, phrases, embedder), args.output
    elif args.command == "check_add_missing":
        with open(args.phrase_emb, "rb") as f:
            table = pickle.load(f)
        with open(args.label) as f:
            phrases = collect_phrases(json.load(f), skip=table)
        print(phrases)
        table, output = embed_into(table, phrases, embedder), args.phrase_emb
    else:
        with open(args.input, "rb") as f:
            labels = [str(c) for c in pickle.load(f).classes_]
        table, output = embed_into({}, labels, embedder), args.output
    with open(output, "wb") as f:
        pickle.dump(table, f)
    print(f"{len(table)} embeddings -> {output}")


if __name__ == "__main__":
    main(build_parser().parse_args())
