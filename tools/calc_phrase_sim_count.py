#!/usr/bin/env python3
"""For every phrase the summed occurrence counts of all phrases whose embedding has cosine >= --threshold with it -> {phrase:
count} JSON, the ``phrase_count`` file of SamplePhrasesCountDataset (the reference's utils/data/calc_phrase_sim_count.py: same
arguments, same file formats).  One fused kernel call on the GPU instead of one host cosine_similarity call per phrase; needs
the GPU, there is no fallback.

    python tools/calc_phrase_sim_count.py --phrase_count_path phrase_count.json --embedding_path phrase_emb.pkl
                                          [--threshold 0.5] --output_path phrase_sim_count.json
"""
import argparse
import json
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(args):
    from texttoaudiogrounding_amd.utils.phrase_stats import phrase_sim_count
    with open(args.phrase_count_path) as f:
        phrase_to_count = json.load(f)
    with open(args.embedding_path, "rb") as f:
        phrase_to_emb = pickle.load(f)
    counts = phrase_sim_count(phrase_to_emb, phrase_to_count, threshold=args.threshold)
    os.makedirs(os.path.dirname(os.path.abspath(args.output_path)), exist_ok=True)
    with open(args.output_path, "w") as f:
        json.dump(counts, f, indent=4)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--phrase_count_path", type=str, required=True)
    parser.add_argument("--embedding_path", type=str, required=True)
    parser.add_argument("--threshold", type=float, default=0.5)
    parser.add_argument("--output_path", type=str, required=True)
    main(parser.parse_args())
