#!/usr/bin/env python3
"""profiles/wave_isolation.json from the files the tests write under PINKHIP_WAVE_ISOLATION_RECORD=<prefix>:

    PINKHIP_WAVE_ISOLATION_RECORD=/tmp/rec python -m pytest tests/test_wave_isolation.py tests/test_wave_primitives.py -m "not gpu"
    PINKHIP_WAVE_ISOLATION_RECORD=/tmp/rec python -m pytest tests/test_wave_isolation.py tests/test_wave_primitives.py -m gpu
    python scripts/wave_isolation_record.py /tmp/rec

cases: per kernel instantiation and backend the arrangements run, the placements compared with their solo result, the
placements that differed, the paths the instances took alone; primitives: per backend, primitive and W the lanes compared with
the NumPy reference and the lanes that differed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(prefix):
    rec = {"cases": {}, "primitives": {}}
    for part in ("cases", "primitives"):
        for backend in ("emu", "gpu"):
            with open(f"{prefix}.{part}.{backend}.json") as f:
                rec[part][backend] = json.load(f)
    rec["differing_placements"] = {b: sum(c["differed"] for c in rec["cases"][b].values()) for b in ("emu", "gpu")}
    rec["differing_lanes"] = {b: sum(v[1] for v in rec["primitives"][b].values()) for b in ("emu", "gpu")}
    with open(os.path.join(ROOT, "profiles", "wave_isolation.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(rec["differing_placements"], rec["differing_lanes"])


if __name__ == "__main__":
    main(sys.argv[1])
