#!/usr/bin/env python3
"""k-means over a phrase-embedding pickle -> the cluster-map JSON that AudioSamplePhrasesDataset(neg_samp_stratg="clustering")
reads and the cluster model that KmeansMappingDataset / KmeansMappingEvalDataset read (the reference's
python_scripts/clustering/kmeans_emb.py: same arguments, same JSON).  The fit runs on the GPU (csrc/kmeans.hip); there is no
fallback, and neither sklearn nor joblib is needed.

    python tools/kmeans_emb.py -e phrase_emb.pkl -nc 32 -o experiments/kmeans/32.json [--seed 0] [--n_init 1] [--device cuda:0]

writes experiments/kmeans/32_score=<inertia>.json ({cluster index: [phrases]}, indent 2) and experiments/kmeans/32_score=<inertia>.npz
(the centres and settings; ``cluster_model`` of the datasets) beside it.
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
    parser.add_argument("--seed", type=int, default=None, help="random_state of the k-means++ seeding")
    parser.add_argument("--n_init", type=int, default=1, help="runs; the one with the lowest inertia is kept")
    parser.add_argument("--device", type=str, default="cuda:0")
    return parser


def output_paths(output, score):
    """-> (<stem>_score=<score:.0f><suffix>, <stem>_score=<score:.0f>.npz) beside ``output``"""
    out = Path(output)
    stem = out.stem + f"_score={score:.0f}"
    return out.with_name(stem + out.suffix), out.with_name(stem + ".npz")


def main(args):
    from texttoaudiogrounding_amd.utils.phrase_cluster import kmeans_cluster_map
    with open(args.embedding, "rb") as f:
        phrase_to_emb = pickle.load(f)
    result = kmeans_cluster_map(phrase_to_emb, args.n_cluster, random_state=args.seed, n_init=args.n_init, device=args.device)
    map_path, model_path = output_paths(args.output, result["score"])
    map_path.parent.mkdir(parents=True, exist_ok=True)
    result["model"].save(str(model_path))
    with open(map_path, "w") as writer:
        json.dump(result["result"], writer, indent=2)
    print(f"{len(phrase_to_emb)} phrases, {args.n_cluster} clusters, inertia {result['score']:.6g}, {result['model'].n_iter_} "
          f"iterations -> {map_path}, {model_path}")


if __name__ == "__main__":
    main(build_parser().parse_args())
