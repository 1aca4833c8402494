"""Record tests/golden/step_parity_parent.json: per case of tests/step_parity_cases.py the run-length encoded sequence
of C-ABI launches, its per-name counts, and sha256 digests of the classifier and detector outputs, of
``flat_gradients()`` and of the BatchNorm running statistics one training step leaves behind.

Needs an MI355X.  The committed file was recorded with the build that preceded ``ops.Scaled`` (the cases call only what
that build already had); tests/test_step_parity_gpu.py holds every later build to it.
    python tests/golden/make_step_parity_golden.py [output.json]
"""
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import step_parity_cases as cases  # noqa: E402

if __name__ == "__main__":
    got = cases.run_cases(torch.device("cuda:0"))
    for name, g in sorted(got.items()):
        print(name, sum(g["counts"].values()), "launches", {k: v[:12] for k, v in g.items() if isinstance(v, str)})
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "step_parity_parent.json"
    lines = [f" {json.dumps(name)}: {json.dumps(g, sort_keys=True)}" for name, g in sorted(got.items())]   # a case a line
    path.write_text("{\n" + ",\n".join(lines) + "\n}\n")
    print(path, len(got), "cases")
