#!/usr/bin/env python3
"""Phrase token-embedding pickle + label token-embedding pickle -> the phrase-to-event table by BERTScore: a TSV with the columns
``phrase``, ``index`` (the label with the largest F1, in the label pickle's insertion order) and ``sim`` (that F1, float32), the
table of tools/map_phrase_to_event.py.  The reference's utils/data/create_phrase_event_mapping/prepare_phrase_bertscore.py runs
``bert_score.score`` on every (phrase, label) pair; here both pickles hold ``{text: (L, D) array}``, the token embeddings of
each text encoded ONCE (any transformer and layer; the [CLS] / [SEP] rows included unless ``--no_special_tokens``), and one
``utils.bertscore_map.BertScoreMap`` call does the all-pairs greedy matching on the GPU (csrc/bertscore.hip); there is no
fallback.  Parity with the ``bert_score`` package is unpinned (utils/bertscore_map.py says what is and is not the same).

    python tools/prepare_phrase_bertscore.py --phrase_emb phrase_tok.pkl --label_emb as_label_tok.pkl --output phrase_to_event.tsv \\
        [--device cuda:0] [--no_special_tokens]
"""
import argparse
import csv
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--phrase_emb", type=str, required=True, help="pickle of {phrase: (L, D) token embeddings}")
    parser.add_argument("--label_emb", type=str, required=True, help="pickle of {label: (L, D) token embeddings}")
    parser.add_argument("--output", type=str, required=True, help="the TSV to write")
    parser.add_argument("--device", type=str, default="cuda:0")
    parser.add_argument("--no_special_tokens", action="store_true",
                        help="the embeddings carry no [CLS] / [SEP] rows: every token weighs 1")
    return parser


def phrase_table(phrase_to_tok, label_to_tok, device="cuda:0", special_tokens=True):
    """-> [(phrase, index, F1)] in the phrase pickle's order"""
    from texttoaudiogrounding_amd.utils.bertscore_map import BertScoreMap
    mapper = BertScoreMap(list(label_to_tok.values()), device=device, special_tokens=special_tokens)
    mapped = mapper.map(list(phrase_to_tok.values()))
    return list(zip(phrase_to_tok, mapped.best.tolist(), mapped.best_f))


def write_table(rows, output):
    with open(output, "w", newline="") as f:
        writer = csv.writer(f, delimiter="\t", lineterminator="\n")
        writer.writerow(["phrase", "index", "sim"])
        for phrase, index, sim in rows:
            writer.writerow([phrase, index, str(sim)])          # (a numpy float32 prints its shortest exact form)


def main(args):
    with open(args.phrase_emb, "rb") as f:
        phrase_to_tok = pickle.load(f)
    with open(args.label_emb, "rb") as f:
        label_to_tok = pickle.load(f)
    rows = phrase_table(phrase_to_tok, label_to_tok, device=args.device, special_tokens=not args.no_special_tokens)
    write_table(rows, args.output)
    print(f"{len(rows)} phrases, {len(label_to_tok)} labels -> {args.output}")


if __name__ == "__main__":
    main(build_parser().parse_args())
