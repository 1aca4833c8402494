"""Captures tests/golden/stimuli_*.npz from the reference's own functions; run by hand where a checkout of the
reference is at hand, never by the suite:

    python tests/golden/make_stimuli_golden.py --reference /path/to/reference

It imports Utils/dynamic_pitch_tools.py, and compiles ``_apply_fade``, ``_normalize`` and ``synthesize_timbre_waveform``
out of the source of Utils/pitch_range_and_timbre_coverage.ipynb's cells and the ``final_error`` expression out of
Utils/dynamic_pitch_behavior.ipynb's at capture time.  Only arrays are written; rows are at most 0.3 s long."""
import argparse
import ast
import importlib.util
import json
import math
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from tests import stimuli_ref as R  # noqa: E402

GLIDES = [(0.05, 60.0, 500.0, 24000), (0.1, 500.0, 60.0, 16000), (0.3, 60.0, 500.0, 24000), (0.02, 100.0, 200.0, 24000),
          (0.03, 80.0, 300.0, 24000)]
VIBRATOS = [(6.0, 60.0, 220.0, 0.3, 24000), (4.0, 200.0, 220.0, 0.25, 16000)]
TONES = [(440.0, 0.1, 24000, 0.8), (150.0, 0.05, 16000, 1.2)]          # the second one is normalised
TIMBRES = [(220.0, 0.3, 24000), (701.5, 0.1, 16000)]
SEED = 1337
PERIOD_MS = 12.5


def frame_counts(n):
    return sorted({1 + n // 300, 97, 7})


def notebook_cells(path):
    return ["".join(c["source"]) for c in json.loads(Path(path).read_text())["cells"] if c["cell_type"] == "code"]


def notebook_functions(path, names, namespace):
    for source in notebook_cells(path):
        try:
            tree = ast.parse(source)
        except SyntaxError:
            continue
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:
                exec(compile(ast.Module([node], []), str(path), "exec"), namespace)
    missing = [n for n in names if n not in namespace]
    if missing:
        raise SystemExit(f"{path}: {missing} not found")
    return namespace


def notebook_expression(path, target):
    for source in notebook_cells(path):
        try:
            tree = ast.parse(source)
        except SyntaxError:
            continue
        for node in ast.walk(tree):
            if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == target for t in node.targets):
                return compile(ast.Expression(node.value), str(path), "eval")
    raise SystemExit(f"{path}: no assignment to {target}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    root = Path(ap.parse_args().reference)
    spec = importlib.util.spec_from_file_location("dynamic_pitch_tools", root / "Utils" / "dynamic_pitch_tools.py")
    tools = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tools)

    dyn = {}
    for k, (duration, start, end, sr) in enumerate(GLIDES):
        audio, t, curve = tools.generate_glide_waveform(duration, start, end, sr)
        dyn.update({f"glide_{k}_audio": audio, f"glide_{k}_t": t, f"glide_{k}_curve": curve})
        for nf in frame_counts(audio.size):
            dyn[f"glide_{k}_ref_{nf}"] = tools.sample_reference_f0(t, curve, nf)
    for k, (rate, depth, base, duration, sr) in enumerate(VIBRATOS):
        audio, t, curve = tools.generate_vibrato_waveform(rate, depth, base, duration, sr)
        dyn.update({f"vibrato_{k}_audio": audio, f"vibrato_{k}_t": t, f"vibrato_{k}_curve": curve})
        for nf in frame_counts(audio.size):
            dyn[f"vibrato_{k}_ref_{nf}"] = tools.sample_reference_f0(t, curve, nf)
    for k, (freq, duration, sr, amplitude) in enumerate(TONES):
        curve = np.full(int(duration * sr), freq, dtype=np.float32)
        dyn[f"tone_{k}_audio"] = tools.synthesize_from_f0_curve(curve, sr, amplitude)
    dyn["glides"], dyn["vibratos"], dyn["tones"] = np.array(GLIDES), np.array(VIBRATOS), np.array(TONES)
    np.savez_compressed(HERE / "stimuli_dynamic.npz", **dyn)

    # metrics: the margin inputs (a 6 Hz vibrato track shifted by 0 / +3 / -2 frames), a delayed linear glide, and
    # the degenerate tracks
    final = notebook_expression(root / "Utils" / "dynamic_pitch_behavior.ipynb", "final_error")
    cases = []
    base = R.shifted_vibrato_track(0)
    for shift in (0, 3, -2):
        cases.append((base, R.shifted_vibrato_track(shift)))
    ramp = np.linspace(60.0, 500.0, 64).astype(np.float32)
    cases.append((ramp, np.concatenate([np.full(4, ramp[0]), ramp[:-4]]).astype(np.float32)))
    cases.append((ramp, (ramp * np.float32(1.03)).astype(np.float32)[:50]))                     # unequal lengths
    cases.append((np.full(32, 220.0, np.float32), base[:32]))                                     # a constant reference
    cases.append((np.concatenate([ramp[:-1], [0.0]]).astype(np.float32), ramp))                  # ref[-1] == 0
    met = {"n_cases": np.array(len(cases)), "period_ms": np.array(PERIOD_MS)}
    for k, (ref, pred) in enumerate(cases):
        L = min(ref.size, pred.size)
        prediction, reference = pred[:L], ref[:L]
        met[f"ref_{k}"], met[f"pred_{k}"] = ref, pred
        met[f"out_{k}"] = np.array([tools.rms_cents_error(ref, pred),
                                    tools.estimate_tracking_delay_ms(ref, pred, PERIOD_MS),
                                    tools.compute_overshoot_cents(ref, pred),
                                    eval(final, {"np": np, "prediction": prediction, "reference": reference,
                                                 "float": float, "max": max})], np.float64)
    np.savez_compressed(HERE / "stimuli_metrics.npz", **met)

    from typing import Any, Dict, Tuple
    from pitchextractor_amd.stimuli import TIMBRE_PROFILES as profiles          # the notebook's CONFIG values
    ns = {"np": np, "math": math, "Dict": Dict, "Any": Any, "Tuple": Tuple, "rng": np.random.default_rng(SEED)}
    notebook_functions(root / "Utils" / "pitch_range_and_timbre_coverage.ipynb",
                       ["_apply_fade", "_normalize", "synthesize_timbre_waveform"], ns)
    tim = {"rows": np.array(TIMBRES), "seed": np.array(SEED)}
    noise_rng = np.random.default_rng(SEED)                    # the draws the notebook's generator makes, in order
    for k, (freq, duration, sr) in enumerate(TIMBRES):
        for j, (name, profile) in enumerate(profiles.items()):
            audio, t = ns["synthesize_timbre_waveform"](freq, sr, duration, profile)
            tim[f"audio_{k}_{j}"] = audio
            if "snr_db" in profile:
                tim[f"noise_{k}_{j}"] = noise_rng.standard_normal(audio.shape).astype(np.float32)
        tim[f"t_{k}"] = t
    np.savez_compressed(HERE / "stimuli_timbre.npz", **tim)
    for name in ("dynamic", "metrics", "timbre"):
        print(name, (HERE / f"stimuli_{name}.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
