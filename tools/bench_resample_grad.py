"""Cost of the resampler's backward next to the forward launch of the same rows, in one session.

  (a) 256 rows of 2 s at 44.1 kHz -> 24 kHz    pe_resample_forward / ragged forward / pe_resample_backward / ragged backward
  (b) the same at 22.05 kHz                     (the longest fmaf chain among the common rates: 320 terms per sample)
  (c) 256 rows of up to 4 s over {16k, 24k, 44.1k, 48k} -> 24 kHz: ragged forward / ragged backward, padded rows
  (d) for (a) and (b): ``inference.f0_from_wave(sample_rate=...)`` + loss + ``backward()`` through the frozen network of
      bench.py, and the backward launch's share of that step

Every pass runs the launch alone (per-row arrays staged once, outputs allocated once) between two device events over
``--iters`` calls after a warm-up; the passes of a workload take turns for ``--rounds`` rounds, every round is kept and
the median reported.  Bytes: each launch's algorithmic traffic (its input rows read once, its output rows written once)
over its time, next to the rate of a device copy of as many bytes timed in the same session.  Before timing, the
ragged backward is compared with the single-rate one bit for bit.  Writes profiles/bench_resample_grad.json and prints
the JSON line.  Needs a GPU.

    python tools/bench_resample_grad.py [--out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import _lib, inference, ops  # noqa: E402
from pitchextractor_amd.mel import DEFAULT_MEL_PARAMS, MelSpectrogram  # noqa: E402
from pitchextractor_amd.model import JDCNet  # noqa: E402
from pitchextractor_amd.resample import RaggedResampler, Resampler  # noqa: E402

B, TARGET, T = 256, 24000, 192
SEQ_CFG = {"model_type": "bilstm", "num_layers": 4, "dropout": 0.1, "nhead": 8, "dim_feedforward": 1536,
           "max_len": 2048}              # bench.py's model (Configs/config.yml)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def rounds_of(passes, iters, rounds, dev):
    ms = {k: [] for k in passes}
    for fn in passes.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize(dev)
    for _ in range(rounds):
        for name, fn in passes.items():
            ms[name].append(timed(fn, iters))
    return ms


def ragged_launches(rr, x, dy, rates, lengths, y, dx, dev):
    """The ragged forward and backward launches alone, on padded rows: per-row arrays staged once."""
    lib = _lib.load()
    distinct = tuple(sorted(set(rates)))
    h32 = torch.tensor(list(lengths) + [distinct.index(r) for r in rates], dtype=torch.int32)
    d32 = h32.to(dev)
    n = len(rates)
    off_x = torch.arange(n, dtype=torch.int64, device=dev) * x.stride(0)
    off_dx = torch.arange(n, dtype=torch.int64, device=dev) * dx.stride(0)
    plan = rr._get_plan(distinct, dev)
    common = (d32.data_ptr(), d32[n:].data_ptr(), h32.data_ptr(), h32[n:].data_ptr(), n)

    def forward():
        _lib.check(lib.pe_resample_ragged_forward(plan, x.data_ptr(), off_x.data_ptr(), *common, y.data_ptr(),
                                                  y.stride(0), y.shape[1], _lib.stream_ptr()),
                   "pe_resample_ragged_forward")

    def backward():
        _lib.check(lib.pe_resample_ragged_backward(plan, dy.data_ptr(), dy.stride(0), off_dx.data_ptr(), *common,
                                                   dx.data_ptr(), dx.shape[1], _lib.stream_ptr()),
                   "pe_resample_ragged_backward")
    forward._keep = (h32, d32, off_x, off_dx)
    return forward, backward


def copy_pass(n_bytes, dev):
    src = torch.empty(n_bytes // 8, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)                          # n_bytes / 2 read + n_bytes / 2 written


def summary(ms, n_bytes):
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {k: {"ms": med[k], "rounds_ms": v} for k, v in ms.items()}
    for k in med:
        if k not in ("chain_wave_to_loss_and_back",):
            out[k]["TBps"] = n_bytes / (med[k] * 1e-3) / 1e12
    return med, out


def one_rate(rate, gen, net, mel, args, dev):
    lib = _lib.load()
    n = 2 * rate
    rs, rr = Resampler(rate, TARGET), RaggedResampler(TARGET)
    m = rs.out_len(n)
    x = (0.3 * torch.randn(B, n, generator=gen)).to(dev)
    dy = (0.3 * torch.randn(B, m, generator=gen)).to(dev)
    y, dx, dx_r = torch.empty(B, m, device=dev), torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
    plan = rs._get_plan(dev)

    def forward():
        _lib.check(lib.pe_resample_forward(plan, x.data_ptr(), B, n, x.stride(0), y.data_ptr(), y.stride(0), m,
                                           _lib.stream_ptr()), "pe_resample_forward")

    def backward():
        _lib.check(lib.pe_resample_backward(plan, dy.data_ptr(), B, m, dy.stride(0), dx.data_ptr(), dx.stride(0), n,
                                            _lib.stream_ptr()), "pe_resample_backward")
    rforward, rbackward = ragged_launches(rr, x, dy, [rate] * B, [n] * B, y, dx_r, dev)
    backward(); rbackward()
    assert torch.equal(dx, dx_r) and bool(torch.isfinite(dx).all().item()) and bool(dx.any().item())
    n_bytes = 4 * B * (n + m)
    f0 = (torch.rand(B, T, generator=gen) * 300 + 80).to(dev)

    def chain():
        w = x.detach().requires_grad_(True)
        cls, _ = inference.f0_from_wave(net, w, mel_transform=mel, max_frames=T, sample_rate=rate)
        torch.nn.functional.smooth_l1_loss(cls.reshape(B, T), f0).backward()
        return w.grad

    ms = rounds_of({"forward": forward, "ragged_forward": rforward, "backward": backward,
                    "ragged_backward": rbackward, "copy_same_bytes": copy_pass(n_bytes, dev)}, args.iters, args.rounds,
                   dev)
    ms.update(rounds_of({"chain_wave_to_loss_and_back": chain}, args.chain_iters, args.rounds, dev))
    assert not ops.persistent_lstm_error(dev)
    med, passes = summary(ms, n_bytes)
    return {"case": f"{B} rows x 2 s, {rate} Hz -> {TARGET} Hz", "rows": B, "n_in": n, "n_out": m,
            "algorithmic_bytes": n_bytes, "passes": passes,
            "backward_over_forward": med["backward"] / med["forward"],
            "backward_over_ragged_forward": med["ragged_backward"] / med["ragged_forward"],
            "backward_rate_over_copy_rate": med["copy_same_bytes"] / med["backward"],
            "backward_share_of_chain": med["backward"] / med["chain_wave_to_loss_and_back"]}


def mixed(gen, args, dev):
    mix = (16000, 24000, 44100, 48000)
    rates = [mix[k % 4] for k in range(B)]
    lengths = [4 * r - int(torch.randint(0, 4000, (1,), generator=gen)) for r in rates]
    rr = RaggedResampler(TARGET)
    out_lengths = [rr.out_len(r, n) for r, n in zip(rates, lengths)]
    x = torch.zeros(B, max(lengths))
    dy = torch.zeros(B, max(out_lengths))
    for r in range(B):
        x[r, :lengths[r]] = 0.3 * torch.randn(lengths[r], generator=gen)
        dy[r, :out_lengths[r]] = 0.3 * torch.randn(out_lengths[r], generator=gen)
    x, dy = x.to(dev), dy.to(dev)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    forward, backward = ragged_launches(rr, x, dy, rates, lengths, y, dx, dev)
    backward()
    for r in (0, 1, 2, 3):                                  # one row of each rate against the single-rate entry
        alone = ops.resample_backward(Resampler(rates[r], TARGET), dy[r:r + 1, :out_lengths[r]], lengths[r])
        assert torch.equal(dx[r:r + 1, :lengths[r]], alone) and not bool(dx[r, lengths[r]:].any().item())
    n_bytes = 4 * (sum(lengths) + sum(out_lengths))          # rows read and written once; the zero padding is extra
    ms = rounds_of({"ragged_forward": forward, "ragged_backward": backward,
                    "copy_same_bytes": copy_pass(n_bytes, dev)}, args.iters, args.rounds, dev)
    med, passes = summary(ms, n_bytes)
    return {"case": f"{B} rows of up to 4 s over {list(mix)} Hz -> {TARGET} Hz, padded", "rows": B,
            "samples_in": sum(lengths), "samples_out": sum(out_lengths), "algorithmic_bytes": n_bytes,
            "passes": passes, "backward_over_ragged_forward": med["ragged_backward"] / med["ragged_forward"],
            "backward_rate_over_copy_rate": med["copy_same_bytes"] / med["ragged_backward"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chain-iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_resample_grad.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(7)
    torch.manual_seed(1234)
    mel = MelSpectrogram(**DEFAULT_MEL_PARAMS)
    net = JDCNet(num_class=1, sequence_model_config=dict(SEQ_CFG)).to(dev).eval().requires_grad_(False)
    res = {"bench": "resample_grad", "device": torch.cuda.get_device_name(dev), "iters_per_round": args.iters,
           "chain_iters_per_round": args.chain_iters, "rounds": args.rounds,
           "results": [one_rate(44100, gen, net, mel, args, dev), one_rate(22050, gen, net, mel, args, dev),
                       mixed(gen, args, dev)]}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
