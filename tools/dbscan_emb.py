#!/usr/bin/env python3
"""DBSCAN over a phrase-embedding pickle -> the cluster-map JSON that AudioSamplePhrasesDataset(neg_samp_stratg="clustering") and
SpectralMappingDataset / SpectralMappingEvalDataset read (the reference's python_scripts/clustering/dbscan_emb.py: same arguments,
same JSON, noise under the key "-1").  The fit runs on the GPU (csrc/dbscan.hip) on N^2 / 8 bytes of adjacency bits; there is no
fallback, and sklearn is not needed.  --eps (cosine distance) and --min_samples default to sklearn's 0.5 and 5, which the
reference's script uses.

    python tools/dbscan_emb.py -e phrase_emb.pkl -o experiments/dbscan/map.json [--eps 0.5] [--min_samples 5] [--device cuda:0]
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
    parser.add_argument("--output", "-o", type=str, required=True, help="e.g., experiments/256.json")
    parser.add_argument("--eps", type=float, default=0.5, help="largest cosine distance between neighbours")
    parser.add_argument("--min_samples", type=int, default=5, help="neighbours (the row itself included) that make a core row")
    parser.add_argument("--device", type=str, default="cuda:0")
    return parser


def main(args):
    from texttoaudiogrounding_amd.utils.phrase_cluster import dbscan_cluster_map
    with open(args.embedding, "rb") as f:
        phrase_to_emb = pickle.load(f)
    result = dbscan_cluster_map(phrase_to_emb, eps=args.eps, min_samples=args.min_samples, device=args.device)
    output = Path(args.output)
    output.parent.mkdir(parents=True, exist_ok=True)
    with open(output, "w") as writer:
        json.dump(result["result"], writer, indent=2)
    model = result["model"]
    print(f"{len(phrase_to_emb)} phrases, {len(result['result']) - ('-1' in result['result'])} clusters, "
          f"{len(result['result'].get('-1', []))} noise phrases, {model.core_sample_indices_.size} core rows, {model.n_passes_} passes "
          f"-> {output}")


if __name__ == "__main__":
    main(build_parser().parse_args())
