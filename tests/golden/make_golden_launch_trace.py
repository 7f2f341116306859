#!/usr/bin/env python3
"""Fixture of the launch sequences of the four whole-encoder autograd nodes (tests/launch_trace.py has the cases and the
recorder).  Data only: per case the list of [C-ABI entry, integer / float arguments and NULL-ness of the pointers, stream].

    python tests/golden/make_golden_launch_trace.py        (needs the MI355X; run it at the commit whose launches are the norm)

Writes tests/golden/encoder_launch_trace.json.  The script uses only ``lib._lib`` and the public model classes, so it runs
unchanged before and after a change of functions.py: record at the parent commit, replay
(tests/test_gpu_encoder_launch_trace.py) at the new one.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import launch_trace as LT  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "encoder_launch_trace.json")
    dev = torch.device("cuda:0")
    traces = {name: run(dev) for name, run in LT.CASES.items()}
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n  ' + ",\n  ".join(json.dumps(e, separators=(",", ":")) for e in t) + "\n ]"
                                   for k, t in traces.items()) + "\n}\n")
    print({k: len(t) for k, t in traces.items()})
    seen = {e[0] for t in traces.values() for e in t}
    for group in LT.COVERAGE:
        assert seen & set(group), f"no case launches {' / '.join(group)}"
    assert any(e[2] == "side" for t in traces.values() for e in t), "no case launches on the side stream"


if __name__ == "__main__":
    main()
