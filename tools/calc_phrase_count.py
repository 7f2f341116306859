#!/usr/bin/env python3
"""Occurrences of every phrase in a label JSON -> {phrase: count} JSON (the reference's utils/data/calc_phrase_count.py: same
arguments, same file formats).

    python tools/calc_phrase_count.py --input label.json --output phrase_count.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(args):
    from texttoaudiogrounding_amd.utils.phrase_stats import phrase_count
    with open(args.input) as f:
        counts = phrase_count(json.load(f))
    with open(args.output, "w") as f:
        json.dump(counts, f, indent=4)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--input", type=str, required=True)
    parser.add_argument("--output", type=str, required=True)
    main(parser.parse_args())
