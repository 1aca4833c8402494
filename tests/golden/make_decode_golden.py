"""Generate tests/golden/pitch_metrics_golden.npz from the reference's own evaluation helpers.

    python tests/golden/make_decode_golden.py <reference checkout>

The reference's ``Utils/dynamic_pitch_tools.py`` is imported, not copied: for a few seeded (reference, prediction)
F0 tracks the file records what ``rms_cents_error`` returned and what ``circular_cents_distance`` gave on the voiced
frames (``hz_to_cents`` of the clipped prediction minus that of the reference, both float32 as the reference
computes them).  The tracks are stored too, so the tests need nothing but this file.
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SEEDS = (11, 12, 13, 14, 15)


def make_pair(seed: int):
    """(ref, pred) float32 tracks.  seed 13: no voiced frame; seed 14: unequal lengths; seed 15: wild errors."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(300, 500))
    ref = np.linspace(rng.uniform(60.0, 250.0), rng.uniform(120.0, 500.0), n)
    gap = int(rng.integers(0, n - 40))
    ref[gap:gap + int(rng.integers(10, 31))] = 0.0
    if seed == 13:
        ref[:] = 0.0
    spread = 400.0 if seed == 15 else 30.0
    pred = np.where(ref > 0, ref, 110.0) * 2.0 ** (rng.normal(0.0, spread, n) / 1200.0)
    octave = rng.choice(n, 12, replace=False)
    pred[octave[:6]] *= 2.0
    pred[octave[6:]] *= 0.5
    pred[rng.choice(n, 10, replace=False)] = 0.0          # misses in voiced frames, agreement in the gap
    voiced_guess = rng.random(n) < 0.9
    pred = np.where((ref > 0) | voiced_guess, pred, 0.0)   # some frames of the gap are called voiced
    if seed == 14:
        pred = pred[:n - 57]
    return ref.astype(np.float32), pred.astype(np.float32)


def main(reference_root: str) -> None:
    spec = importlib.util.spec_from_file_location("dynamic_pitch_tools",
                                                  Path(reference_root) / "Utils" / "dynamic_pitch_tools.py")
    tools = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tools)
    out = {"seeds": np.asarray(SEEDS, dtype=np.int64)}
    for k, seed in enumerate(SEEDS):
        ref, pred = make_pair(seed)
        out[f"ref_{k}"], out[f"pred_{k}"] = ref, pred
        out[f"rms_{k}"] = np.float64(tools.rms_cents_error(ref, pred))
        n = min(len(ref), len(pred))
        r, p = ref[:n], pred[:n]
        m = r > 0
        circ = tools.circular_cents_distance(tools.hz_to_cents(np.clip(p[m], a_min=1e-5, a_max=None)),
                                             tools.hz_to_cents(r[m]))
        out[f"circ_{k}"] = np.asarray(circ, dtype=np.float32)
    np.savez_compressed(HERE / "pitch_metrics_golden.npz", **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
