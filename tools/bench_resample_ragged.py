"""Ragged multi-rate resample launch against the single-rate kernel, timed with HIP events, old and new interleaved.

(a) config[4]'s front end: 256 rows x 4 s at 44.1 kHz -> 24 kHz, ``pe_resample_forward`` vs one ragged launch (all
    rows at one rate, y_width = the output length).
(b) 256 rows of up to 4 s mixed over {16k, 24k, 44.1k, 48k}: one single-rate launch per rate on the gathered rows,
    then a scatter into the padded batch buffer, vs one ragged launch writing that buffer directly.
Each round times ``reps`` back-to-back calls of one variant, then of the other; prints one JSON line (median and
min / max per-call milliseconds over the rounds) and writes it to --out if given."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pitchextractor_amd import _lib  # noqa: E402
from pitchextractor_amd.resample import RaggedResampler, Resampler  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
B, TARGET = 256, 24000
lib = _lib.load()
gen = torch.Generator(device="cpu").manual_seed(0)


def ragged_call(rr, x, rates, lengths, y):
    """The launch alone: per-row arrays staged once, outside the timed region."""
    distinct = tuple(sorted(set(rates)))
    ridx = [distinct.index(r) for r in rates]
    h32 = torch.tensor(list(lengths) + ridx, dtype=torch.int32)
    d32 = h32.to(dev)
    d64 = torch.arange(B, dtype=torch.int64, device=dev) * x.stride(0)
    plan = rr._get_plan(distinct, dev)
    args_ = (plan, x.data_ptr(), d64.data_ptr(), d32.data_ptr(), d32[B:].data_ptr(), h32.data_ptr(),
             h32[B:].data_ptr(), B, y.data_ptr(), y.stride(0), y.shape[1])

    def run():
        _lib.check(lib.pe_resample_ragged_forward(*args_, _lib.stream_ptr()), "pe_resample_ragged_forward")
    run._keep = (h32, d32, d64)
    return run


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(name, old, new):
    for _ in range(3):
        old(); new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(args.rounds):
        t_old.append(timed(old, args.reps))
        t_new.append(timed(new, args.reps))
    s = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}  # noqa: E731
    return {"case": name, "old": s(t_old), "new": s(t_new), "new_over_old": float(np.median(t_new) / np.median(t_old))}


results = []
# (a) one rate
n = 4 * 44100
x = (0.3 * torch.randn(B, n, generator=gen)).to(dev)
rs = Resampler(44100, TARGET)
n_out = rs.out_len(n)
y_old = torch.empty(B, n_out, device=dev)
y_new = torch.empty(B, n_out, device=dev)
plan = rs._get_plan(dev)


def old_a():
    _lib.check(lib.pe_resample_forward(plan, x.data_ptr(), B, n, x.stride(0), y_old.data_ptr(), y_old.stride(0),
                                       n_out, _lib.stream_ptr()), "pe_resample_forward")


new_a = ragged_call(RaggedResampler(TARGET), x, [44100] * B, [n] * B, y_new)
old_a(); new_a()
assert torch.equal(y_old, y_new)
results.append(compare("a: 256 x 4 s, 44.1 kHz -> 24 kHz", old_a, new_a))

# (b) four rates in one batch
mix = (16000, 24000, 44100, 48000)
rates = [mix[k % 4] for k in range(B)]
lengths = [4 * r - int(torch.randint(0, 4000, (1,), generator=gen)) for r in rates]
xm = torch.zeros(B, 4 * 48000)
for r, m in enumerate(lengths):
    xm[r, :m] = 0.3 * torch.randn(m, generator=gen)
xm = xm.to(dev)
rr = RaggedResampler(TARGET)
width = max(rr.out_len(r, m) for r, m in zip(rates, lengths))
yb_old = torch.empty(B, width, device=dev)
yb_new = torch.empty(B, width, device=dev)
groups = []
for rate in mix:
    rows = [k for k in range(B) if rates[k] == rate]
    groups.append((rate, torch.tensor(rows, device=dev), max(lengths[k] for k in rows)))
resamplers = {rate: Resampler(rate, TARGET) for rate in mix}


def old_b():
    yb_old.zero_()
    for rate, rows, m in groups:
        part = resamplers[rate](xm.index_select(0, rows)[:, :m])
        yb_old[:, :part.shape[1]].index_copy_(0, rows, part)


new_b = ragged_call(rr, xm, rates, lengths, yb_new)
old_b(); new_b()
for k in range(B):                                      # same samples wherever the row has output
    m = rr.out_len(rates[k], lengths[k])
    assert torch.equal(yb_old[k, :m], yb_new[k, :m]), k
results.append(compare("b: 256 rows over {16k, 24k, 44.1k, 48k} -> 24 kHz", old_b, new_b))

line = json.dumps({"bench": "resample_ragged", "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
                   "reps": args.reps, "results": results})
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
