#!/usr/bin/env python3
"""Phrase-embedding pickle + label-embedding pickle -> the phrase-to-event table: a TSV with the columns ``phrase``, ``index`` (the
most similar label, in the label pickle's insertion order) and ``sim`` (that cosine similarity, float32).  The reference's
utils/data/map_phrase_to_event.py, same three arguments; it calls sklearn's cosine_similarity once per phrase on the host, here ONE
``utils.label_map.LabelMap`` call maps all phrases on the GPU (csrc/label_map.hip); there is no fallback.

    python tools/map_phrase_to_event.py --phrase_emb phrase_emb.pkl --label_emb as_label_emb.pkl --output phrase_to_event.tsv [--device cuda:0]
"""
import argparse
import csv
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--phrase_emb", type=str, required=True, help="pickle of {phrase: vector}")
    parser.add_argument("--label_emb", type=str, required=True, help="pickle of {label: vector}")
    parser.add_argument("--output", type=str, required=True, help="the TSV to write")
    parser.add_argument("--device", type=str, default="cuda:0")
    return parser


def phrase_table(phrase_to_emb, label_to_emb, device="cuda:0"):
    """-> [(phrase, index, sim)] in the phrase pickle's order"""
    from texttoaudiogrounding_amd.utils.label_map import LabelMap, stack_embeddings
    mapped = LabelMap(stack_embeddings(label_to_emb), device=device).map(stack_embeddings(phrase_to_emb))
    return list(zip(phrase_to_emb, mapped.best.tolist(), mapped.best_sim))


def write_table(rows, output):
    with open(output, "w", newline="") as f:
        writer = csv.writer(f, delimiter="\t", lineterminator="\n")
        writer.writerow(["phrase", "index", "sim"])
        for phrase, index, sim in rows:
            writer.writerow([phrase, index, str(sim)])          # (a numpy float32 prints its shortest exact form)


def main(args):
    with open(args.phrase_emb, "rb") as f:
        phrase_to_emb = pickle.load(f)
    with open(args.label_emb, "rb") as f:
        label_to_emb = pickle.load(f)
    rows = phrase_table(phrase_to_emb, label_to_emb, device=args.device)
    write_table(rows, args.output)
    print(f"{len(rows)} phrases, {len(label_to_emb)} labels -> {args.output}")


if __name__ == "__main__":
    main(build_parser().parse_args())
