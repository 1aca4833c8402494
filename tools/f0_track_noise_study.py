"""Which stage of the F0 tracker turns float32 rounding into cents (CPU only, float64 restatement with noise injected).

For one natural test input per configuration the float64 restatement is rerun with Gaussian noise added to one stage
at a time, at the size float32 leaves there: (a) on r, with the rms of the float32 restatement's own r deviation;
(b) on every value of the sinc interpolation, sigma 5e-8 (half a float32 rounding of a value near 1).  Printed: the
largest contour deviation in cents over the voiced frames, minimum / median / maximum over the draws.  Result recorded
in DESIGN.md section 13: (a) gives medians of 0.6e-3 .. 1.6e-3 cents and never more than 4.2e-3; (b) gives medians of
3e-3 .. 7e-3 cents and spreads over a factor of 4 to 15 from draw to draw (up to 2.1e-2), because the last parabolic
steps of the refinement divide a difference of interpolated values by their second difference at h = 1/8 lag.  Hence
the kernel refines in double.

    python tools/f0_track_noise_study.py [draws]
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tests import f0_track_ref as R  # noqa: E402


def study(sr, hop, min_pitch, draws):
    y = R.natural_inputs(sr)[1]
    a = R.track(y, sr, hop, min_pitch=min_pitch)
    b = R.track(y, sr, hop, dtype=np.float32, min_pitch=min_pitch)
    r_rms = float((a["r"] - b["r"].astype(np.float64)).std())
    print(f"sr {sr} hop {hop} min_pitch {min_pitch}: float32 restatement contour {R.deviation(a, b)['contour_cents']:.2e} "
          f"cents, r deviation rms {r_rms:.1e}")
    corr, sinc = R.frame_correlations, R.sinc_interp
    for stage, sigma in (("r", r_rms), ("sinc", 5e-8)):
        worst = []
        for d in range(draws):
            rng = np.random.default_rng(d)

            def noisy_corr(x, c, dtype=np.float64):
                r, inten, silent, lp, gp = corr(x, c, dtype)
                r = r + rng.standard_normal(r.shape) * sigma
                r[:, 0] = 1
                r[silent] = 0
                return r, inten, silent, lp, gp

            def noisy_sinc(r, rows, x, depth, hw):
                v = sinc(r, rows, x, depth, hw)
                return v + rng.standard_normal(v.shape) * sigma

            if stage == "r":
                R.frame_correlations = noisy_corr
            else:
                R.sinc_interp = noisy_sinc
            try:
                n = R.track(y, sr, hop, min_pitch=min_pitch)
            finally:
                R.frame_correlations, R.sinc_interp = corr, sinc
            worst.append(R.deviation(a, n)["contour_cents"])
        w = np.array(worst)
        print(f"   noise on {stage:4s} sigma {sigma:.1e}: contour cents min {w.min():.2e} median {np.median(w):.2e} "
              f"max {w.max():.2e} over {draws} draws")


if __name__ == "__main__":
    n_draws = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    for cfg in R.GPU_CONFIGS:
        study(*cfg[:3], n_draws)
