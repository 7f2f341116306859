#!/usr/bin/env python3
"""Event-based and segment-based scores of a prediction file against a grounding ground truth: the arguments of the reference's
python_scripts/evaluation/evaluate_sed_eval.py, on the host (utils/sed_metrics.py; no GPU, no sed_eval / dcase_util).

ground_truth   JSON: ``[{"audiocap_id": ..., "phrases": [{"start_index": ..., "segments": [[onset, offset], ...]}, ...]}, ...]``;
               every (clip, phrase) pair is the file ``f"{audiocap_id}_{start_index}"`` with one label, (0, 0) rows are dropped
prediction     TSV with the columns ``filename``, ``onset``, ``offset`` (further columns are ignored); files the ground truth
               does not name are not evaluated
event_output, segment_output   the two reports, plain ``key: value`` lines (NOT sed_eval's report layout)

    python tools/evaluate_sed_eval.py GROUND_TRUTH.json PREDICTION.tsv EVENT.txt SEGMENT.txt [--t_collar 0.2] [--time_resolution 1.0]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_ground_truth(path):
    table = {}
    for audio_item in json.load(open(path)):
        for phrase_item in audio_item["phrases"]:
            rows = [[float(on), float(off)] for on, off in phrase_item["segments"] if not (on == 0 and off == 0)]
            if rows:                                            # (the reference's DataFrame has no row, hence no file, otherwise)
                table.setdefault(f"{audio_item['audiocap_id']}_{phrase_item['start_index']}", []).extend(rows)
    return {k: np.array(v, dtype=np.float64).reshape(-1, 2) for k, v in table.items()}


def read_prediction(path):
    table = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f, delimiter="\t"):
            if row.get("onset") in (None, "") or row.get("offset") in (None, ""):
                continue                                        # (a file listed without an event)
            table.setdefault(row["filename"], []).append([float(row["onset"]), float(row["offset"])])
    return {k: np.array(v, dtype=np.float64).reshape(-1, 2) for k, v in table.items()}


def report(title, scores, counts, settings):
    lines = [title] + [f"{k}: {v}" for k, v in settings.items()] + [f"{k}: {int(v)}" for k, v in counts.items()]
    lines += [f"{k}: {float(v):.6f}" for k, v in scores.items()]
    return "\n".join(lines) + "\n"


def evaluate(ground_truth, prediction, event_output, segment_output, t_collar=0.2, time_resolution=1.0):
    from texttoaudiogrounding_amd.utils import sed_metrics
    gt, pred = read_ground_truth(ground_truth), read_prediction(prediction)
    out = sed_metrics.compute_sed_eval(gt, pred, t_collar=t_collar, time_resolution=time_resolution)
    ev_tp, seg_tp, seg_fp, seg_fn, seg_n, n_sys, n_ref = (int(v) for v in out["counts"])
    for path in (event_output, segment_output):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(event_output, "w") as f:
        f.write(report("event-based, optimal matching, one label", out["event"],
                       {"files": len(gt), "n_ref": n_ref, "n_sys": n_sys, "tp": ev_tp, "fp": n_sys - ev_tp, "fn": n_ref - ev_tp},
                       {"t_collar": t_collar, "percentage_of_length": 0.2}))
    with open(segment_output, "w") as f:
        f.write(report("segment-based, one label", out["segment"],
                       {"files": len(gt), "segments": seg_n, "tp": seg_tp, "fp": seg_fp, "fn": seg_fn},
                       {"time_resolution": time_resolution}))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ground_truth")
    ap.add_argument("prediction")
    ap.add_argument("event_output")
    ap.add_argument("segment_output")
    ap.add_argument("--t_collar", type=float, default=0.2)
    ap.add_argument("--time_resolution", type=float, default=1.0)
    args = ap.parse_args(argv)
    evaluate(args.ground_truth, args.prediction, args.event_output, args.segment_output, args.t_collar, args.time_resolution)


if __name__ == "__main__":
    main()
