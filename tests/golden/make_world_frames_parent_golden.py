"""Record tests/golden/world_frames_parent_bits.json: SHA-256 digests of the float32 bytes ``world.cheaptrick_ragged``,
``world.d4c_ragged`` (aperiodicity and band values) and ``world.resynthesize(..., ap="d4c")`` leave on the cases of
tests/world_frames_cases.py, per case and row.

Needs an MI355X.  The committed file was recorded with the build that preceded csrc/world_frames.h, when cheaptrick.hip
and d4c.hip each held a frame plan, a DC correction and an interval sum of their own (the cases call only what that
build already had); tests/test_world_frames_parity_gpu.py holds every later build to it.
    python tests/golden/make_world_frames_parent_golden.py [output.json]
"""
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import world_frames_cases as cases  # noqa: E402

if __name__ == "__main__":
    got = cases.run_cases(torch.device("cuda:0"))
    assert sorted(got) == cases.CASES
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "world_frames_parent_bits.json"
    path.write_text(json.dumps(got, indent=1, sort_keys=True) + "\n")
    print(path, len(got), "cases,", sum(len(v) for v in got.values()), "rows")
