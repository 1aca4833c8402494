"""Record tests/golden/snr_mix_parent_bits.json: digests of the bits ``noise.mix_at_snr`` / ``pe_noise_mix`` and
``stimuli.finish`` leave on the cases of tests/snr_mix_cases.py.

Needs an MI355X.  The committed file was recorded with the build that preceded the shared SNR mix of csrc/snr_mix.h (the
cases call only what that build already had); tests/test_snr_mix_parity_gpu.py holds every later build to it.
    python tests/golden/make_snr_mix_parent_golden.py [output.json]
"""
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import snr_mix_cases as cases  # noqa: E402

if __name__ == "__main__":
    got = cases.run_cases(torch.device("cuda:0"))
    for name, (_, st) in sorted(got.items()):
        print(name, "peaks", [round(v, 4) for v in st[:, 0].cpu().tolist()])
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "snr_mix_parent_bits.json"
    path.write_text(json.dumps(cases.digests(got), indent=1, sort_keys=True) + "\n")
    print(path, len(got), "cases")
