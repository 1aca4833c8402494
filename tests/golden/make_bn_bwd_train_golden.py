"""Record tests/golden/bn_bwd_train_bits.json: digests of the bits the TRAIN-mode BatchNorm backward passes
(pe_bn_act_pool_bwd / pe_bn_act_pool_tap_bwd) leave on the cases of tests/bn_bwd_cases.py.

Needs an MI355X.  The committed file was recorded with the build that preceded the eval mode of these passes (the
cases call them through arguments that build already had); tests/test_bn_eval_bwd_gpu.py holds every later build to it.
    python tests/golden/make_bn_bwd_train_golden.py [output.json]
"""
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from pitchextractor_amd import ops  # noqa: E402
from tests import bn_bwd_cases as cases  # noqa: E402

if __name__ == "__main__":
    dev = torch.device("cuda:0")
    out = {name: {k: cases.digest(v) for k, v in cases.run_train_case(ops, name, dev).items()}
           for name in sorted(cases.CASES)}
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "bn_bwd_train_bits.json"
    path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(path, len(out), "cases")
