"""Device cost of the pitch-modulation stage (``pitchextractor_amd.pitch_mod``).

Reports, from one session, on a B = 256 batch of 2-s rows at 24 kHz and hop 300 (161 kept frames, every row warped
with a vibrato, a flutter, a drift and a glide): the wave kernel per quality, kaiser_fast with its table read from L2
and from the copy in LDS, and the label kernel (HIP events around ``reps`` back-to-back launches of the entry point,
plans and tables made before); ``PitchModulator.apply`` with its host work (wall clock around a synchronize) and the host
cost of ``draw``; and the fp32 training step of the flagship batch (bench.py as a child process, before and after the
rest), which the stage is given as a share of.  Writes profiles/bench_pitch_mod.json and prints the JSON line.  Needs a
GPU.  Not a gate.

    python tools/bench_pitch_mod.py [--reps 30] [--no-train-step] [--out PATH]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench_cheaptrick as bc  # noqa: E402
from pitchextractor_amd import _lib, pitch_mod as PM  # noqa: E402
from pitchextractor_amd.pitch_shift import RES_TYPES  # noqa: E402

SR, HOP, BATCH, SECONDS = 24000, 300, 256, 2.0
CONFIG = {"p": 1.0, "vibrato": {"p": 1.0}, "flutter": {"p": 1.0}, "drift": {"p": 1.0}, "glide": {"p": 1.0}}


def event_ms(fn, reps):
    """Mean device time of one ``fn()`` over ``reps`` back-to-back calls, and the smallest of five such means."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        means.append(a.elapsed_time(b) / reps)
    return float(np.median(means)), float(np.min(means))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_pitch_mod.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pitch_mod: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    step_before = None if a.no_train_step else bc.training_step_ms()
    n = int(SR * SECONDS)
    rng = np.random.default_rng(0)
    x = torch.from_numpy((0.1 * rng.standard_normal((BATCH, n))).astype(np.float32)).to(dev)
    lengths, crops = [n] * BATCH, [0] * BATCH
    pm = PM.PitchModulator(CONFIG, SR, HOP, seed=0)
    plan = pm.draw(BATCH)
    spans, counts = PM.frame_spans(lengths, crops, HOP)
    k = PM.kernel_consts()
    res = {"sr": SR, "hop": HOP, "batch": BATCH, "seconds_per_row": SECONDS, "frames_per_row": int(counts[0]),
           "warped_samples": int((spans[:, 1] - spans[:, 0] - 1).sum()), "tile": k["tile"], "block": k["block"],
           "sinusoids_per_row": 3, "default_table_in_lds": PM.TABLE_IN_LDS}
    pl = PM._plan(lengths, [r * n for r in range(BATCH)], [r * n for r in range(BATCH)], spans, plan.mods, SR, HOP,
                  "bench_pitch_mod")
    meta_d, params_d = torch.from_numpy(pl["meta"]).to(dev), torch.from_numpy(pl["params"]).to(dev)
    y = torch.empty_like(x)
    lib = _lib.load()

    def wave(quality, in_lds):
        table = PM.filter_table(quality, dev)
        q = list(RES_TYPES).index(quality)
        return lambda: _lib.check(lib.pe_pitch_mod_wave(
            x.data_ptr(), meta_d.data_ptr(), pl["meta"].ctypes.data, params_d.data_ptr(), pl["params"].ctypes.data,
            BATCH, table.data_ptr(), q, int(in_lds), y.data_ptr(), _lib.stream_ptr()), "pe_pitch_mod_wave")

    res["wave_kernel_ms"] = {}
    for quality, in_lds in (("kaiser_fast", False), ("kaiser_fast", True), ("kaiser_best", False)):
        med, low = event_ms(wave(quality, in_lds), a.reps)
        res["wave_kernel_ms"][f"{quality}_{'lds' if in_lds else 'l2'}_table"] = {"median": med, "min": low}
    f0 = torch.full((BATCH, 192), 200.0, device=dev)
    sil = torch.zeros_like(f0)
    f0_out, sil_out = torch.empty_like(f0), torch.empty_like(sil)
    med, low = event_ms(lambda: _lib.check(lib.pe_pitch_mod_labels(
        f0.data_ptr(), sil.data_ptr(), meta_d.data_ptr(), pl["meta"].ctypes.data, params_d.data_ptr(),
        pl["params"].ctypes.data, BATCH, HOP, 192, f0_out.data_ptr(), sil_out.data_ptr(), _lib.stream_ptr()),
        "pe_pitch_mod_labels"), a.reps)
    res["labels_kernel_ms"] = {"median": med, "min": low}
    res["apply_ms_median"], res["apply_ms_min"] = bc.wall_ms(lambda: pm.apply(x, lengths, crops, f0, sil, plan), a.reps)
    res["draw_ms_median"], res["draw_ms_min"] = bc.wall_ms(lambda: pm.draw(BATCH), a.reps)
    if not a.no_train_step:
        step_after = bc.training_step_ms()
        res["training_step_ms_fp32_batch256_before"], res["training_step_ms_fp32_batch256_after"] = step_before, step_after
        step = 0.5 * (step_before + step_after)
        fast = res["wave_kernel_ms"]["kaiser_fast_lds_table" if PM.TABLE_IN_LDS["kaiser_fast"] else
                                     "kaiser_fast_l2_table"]["median"]
        res["kernels_to_training_step_ratio"] = (fast + res["labels_kernel_ms"]["median"]) / step
        res["apply_to_training_step_ratio"] = res["apply_ms_median"] / step
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
