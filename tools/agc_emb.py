#!/usr/bin/env python3
"""Average-linkage clustering over a phrase-embedding pickle -> the cluster-map JSON that
AudioSamplePhrasesDataset(neg_samp_stratg="clustering") and SpectralMappingDataset / SpectralMappingEvalDataset read (the reference's
python_scripts/clustering/agc_emb.py: same arguments, same JSON).  The fit runs on the GPU (csrc/agc.hip) without the N x N distance
matrix; there is no fallback, and sklearn is not needed.

    python tools/agc_emb.py -e phrase_emb.pkl -nc 256 -o experiments/agc/256.json [--device cuda:0]
"""
import argparse
import json
import os
import pickle
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--embedding", "-e", type=str, required=True, help="pickle of {phrase: vector}")
    parser.add_argument("--n_cluster", "-nc", type=int, required=True)
    parser.add_argument("--output", "-o", type=str, required=True, help="e.g., experiments/256.json")
    parser.add_argument("--device", type=str, default="cuda:0")
    return parser


def main(args):
    from texttoaudiogrounding_amd.utils.phrase_cluster import agc_cluster_map
    with open(args.embedding, "rb") as f:
        phrase_to_emb = pickle.load(f)
    result = agc_cluster_map(phrase_to_emb, args.n_cluster, device=args.device)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    with open(output, "w") as writer:
        json.dump(result["result"], writer, indent=2)
    model = result["model"]
    print(f"{len(phrase_to_emb)} phrases, {len(result['result'])} clusters, {model.n_rounds_} rounds -> {output}")


if __name__ == "__main__":
    main(build_parser().parse_args())
