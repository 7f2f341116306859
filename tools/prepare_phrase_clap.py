#!/usr/bin/env python3
"""Phrase / label embeddings from the text side of a trained audio-text retrieval model, as the ``{text: float32 vector}``
pickles that tools/map_phrase_to_event.py, tools/kmeans_emb.py and the other clustering tools read.  The reference's
utils/data/create_text_embedding/prepare_phrase_clap.py builds the whole ``AudioTextClip`` and runs its ``Bert`` text encoder
(+ ``text_proj`` and the model's normalisation with ``--with_proj``); here ``utils.text_embed.RetrievalTextEncoder`` loads only
the text side of ``<experiment_path>/models/trained_model.pth`` and runs on the HIP text tower through ``PhraseEmbedder``.
Deviations: batches hold ``--batch_size`` phrases of similar token count and are padded to their own longest phrase, not to
``max_text_length`` (the result for valid tokens does not depend on the padding); truncation at min(max_text_length, 64) tokens;
the tokenizer must resolve locally.  No fallback.

    python tools/prepare_phrase_clap.py phrase --experiment_path EXP --phrase_input label.json --output phrase_emb.pkl \\
        [--debug] [--batch_size 128] [--with_proj]
    python tools/prepare_phrase_clap.py add_phrase --experiment_path EXP --extra_phrase extra.txt --phrase_emb in.pkl --output out.pkl
    python tools/prepare_phrase_clap.py label --experiment_path EXP --label_encoder_input label_encoder.pkl --output label_emb.pkl
"""
import argparse
import json
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.prepare_phrase_sbert import collect_phrases, embed_into  # noqa: E402


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = parser.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("--experiment_path", type=str, required=True, help="holds models/config.json and models/trained_model.pth")
        p.add_argument("--output", type=str, required=True)
        p.add_argument("--batch_size", type=int, default=128, help="phrases per batch")
        p.add_argument("--with_proj", action="store_true", help="text_proj and x / (|x| + 1e-7) clipped to +-1e3 on top of [CLS]")
        p.add_argument("--device", type=str, default="cuda:0")
    p = sub.add_parser("phrase", help="the unique phrases of a label JSON -> pickle")
    p.add_argument("--phrase_input", type=str, required=True)
    p.add_argument("--debug", action="store_true", help="the first 51 clips only")
    common(p)
    p = sub.add_parser("add_phrase", help="a pickle + the phrases of a text file (one per line) -> pickle")
    p.add_argument("--extra_phrase", type=str, required=True)
    p.add_argument("--phrase_emb", type=str, required=True)
    common(p)
    p = sub.add_parser("label", help="the classes of a pickled LabelEncoder -> pickle")
    p.add_argument("--label_encoder_input", type=str, required=True)
    common(p)
    return parser


def load_embedder(args):
    from texttoaudiogrounding_amd.utils.text_embed import PhraseEmbedder, RetrievalTextEncoder
    enc, tok, config = RetrievalTextEncoder.from_experiment(args.experiment_path, args.with_proj, args.device)
    max_len = min(int(config["data_loader"]["collate_fn"]["args"].get("max_text_length", 64)), 64)
    return PhraseEmbedder(enc, tok, batch_tokens=args.batch_size * max_len, max_length=max_len)


def main(args, embedder=None):
    embedder = embedder or load_embedder(args)
    table = {}
    if args.command == "phrase":
        with open(args.phrase_input) as f:
            texts = collect_phrases(json.load(f), args.debug)
    elif args.command == "add_phrase":
        with open(args.extra_phrase) as f:
            texts = [line.strip() for line in f.readlines()]
        with open(args.phrase_emb, "rb") as f:
            table = pickle.load(f)
    else:
        with open(args.label_encoder_input, "rb") as f:
            texts = [str(c) for c in pickle.load(f).classes_]
    embed_into(table, texts, embedder)
    with open(args.output, "wb") as f:
        pickle.dump(table, f)
    print(f"{len(table)} embeddings -> {args.output}")


if __name__ == "__main__":
    main(build_parser().parse_args())
