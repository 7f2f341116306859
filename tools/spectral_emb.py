#!/usr/bin/env python3
"""Spectral clustering over a phrase-embedding pickle -> the cluster-map JSON that
AudioSamplePhrasesDataset(neg_samp_stratg="clustering") and SpectralMappingDataset / SpectralMappingEvalDataset read (the reference's
python_scripts/clustering/spectral_emb.py: same arguments, same JSON).  The fit runs on the GPU (csrc/spectral.hip) without the
N x N affinity matrix; there is no fallback, and sklearn is not needed.

    python tools/spectral_emb.py -e phrase_emb.pkl -nc 256 -o experiments/spectral/256.json [--seed 1] [--device cuda:0]
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
    parser.add_argument("--seed", type=int, required=False, default=1)
    parser.add_argument("--device", type=str, default="cuda:0")
    return parser


def main(args):
    from texttoaudiogrounding_amd.utils.phrase_cluster import spectral_cluster_map
    with open(args.embedding, "rb") as f:
        phrase_to_emb = pickle.load(f)
    result = spectral_cluster_map(phrase_to_emb, args.n_cluster, seed=args.seed, device=args.device)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    with open(output, "w") as writer:
        json.dump(result["result"], writer, indent=2)
    model = result["model"]
    print(f"{len(phrase_to_emb)} phrases, {len(result['result'])} clusters, block {model.block_}, {model.n_iter_} iterations, residual "
          f"{model.residuals_[-1] if model.residuals_ else 0.0:.3g} -> {output}")


if __name__ == "__main__":
    main(build_parser().parse_args())
