"""Record tests/golden/bn_family_bits.json: digests of the bits the BatchNorm / LeakyReLU / max-pool passes leave on
the cases of tests/bn_family_cases.py.

Needs an MI355X.  The committed file was recorded with the build that preceded the rewrite of these passes around
shared helpers (PITCHEXTRACTOR_HIP_LIB pointing at that build's library; the cases call only ``ops`` functions that
build already had); tests/test_bn_family_bits_gpu.py holds every later build to it.
    python tests/golden/make_bn_family_golden.py [output.json]
"""
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from pitchextractor_amd import ops  # noqa: E402
from tests import bn_family_cases as cases  # noqa: E402

if __name__ == "__main__":
    dev = torch.device("cuda:0")
    out = {name: {k: cases.digest(v) for k, v in cases.run_case(ops, name, dev).items()}
           for name in sorted(cases.CASES)}
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "bn_family_bits.json"
    path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(path, len(out), "cases")
