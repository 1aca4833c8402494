"""Cost of the mel front end's backward next to its forward and to the frozen loss network it feeds: B = 256 rows of
48 000 samples (2 s at 24 kHz, 161 frames in 192), in one session.

  (a) mel_forward    ``log_mel_batch`` under ``no_grad``: the yardstick (one launch)
  (b) mel_backward   ``ops.mel_backward`` on the same batch (two launches: frames, gather), per call
  (c) network        eval forward + input-gradient backward of the frozen JDCNet on that mel (bench_input_grad's pass b)
  (d) chain          ``inference.f0_from_wave`` + loss + ``backward()`` to the waveform: (a) + (b) + (c) under autograd

Each pass is timed between two device events over ``--iters`` runs after a warm-up; the passes take turns for
``--rounds`` rounds and every round is kept (median reported).  Reports backward / forward and the backward's share of
the chain.  The algorithmic bytes of the backward (wave read, gradient written, grad_out read) over its time are
given as a rate, with the slab traffic of its two launches next to it.

Per kernel: ``--trace-loop`` only runs the backward ``--iters`` times, for a run of its own under
``rocprofv3 --kernel-trace --stats -- python tools/bench_mel_grad.py --trace-loop``; ``--kernel-stats FILE`` (that run's
``*_kernel_stats.csv``) adds the two kernels' average times to the result.  Writes profiles/bench_mel_grad.json and
prints the JSON line.  Needs a GPU.

    python tools/bench_mel_grad.py [--kernel-stats FILE] [--out FILE]
"""
import argparse
import csv
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

B, N, T = 256, 48000, 192
SEQ_CFG = {"model_type": "bilstm", "num_layers": 4, "dropout": 0.1, "nhead": 8, "dim_feedforward": 1536,
           "max_len": 2048}              # bench.py's model (Configs/config.yml)
KERNELS = ("mel_bwd_frames_kernel", "mel_bwd_gather_kernel", "mel_fwd_kernel")


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def kernel_stats(path):
    """Average ms of the mel kernels from a rocprofv3 kernel-stats csv (columns Name, Calls, AverageNs)."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row.get("Name", ""):
                    out[k] = {"calls": int(row["Calls"]), "avg_ms": float(row["AverageNs"]) * 1e-6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-loop", action="store_true", help="only run the backward --iters times (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="kernel-stats csv of a --trace-loop run under rocprofv3")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_mel_grad.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mel = MelSpectrogram(**DEFAULT_MEL_PARAMS)
    g = torch.Generator().manual_seed(7)
    wave = (0.3 * torch.randn(B, N, generator=g)).to(dev)
    grad_out = torch.randn(B, 1, T, mel.n_mels, generator=g).to(dev).transpose(-1, -2)     # as the network returns it
    valid = mel.num_frames(N)

    def mel_forward():
        with torch.no_grad():
            return mel.log_mel_batch(wave, max_frames=T)

    def mel_backward():
        return ops.mel_backward(mel, wave, grad_out)

    if args.trace_loop:
        for _ in range(args.iters):
            mel_forward()
            mel_backward()
        torch.cuda.synchronize(dev)
        return

    torch.manual_seed(1234)
    net = JDCNet(num_class=1, sequence_model_config=dict(SEQ_CFG)).to(dev).eval().requires_grad_(False)
    f0 = (torch.rand(B, T, generator=g) * 300 + 80).to(dev)
    x = mel_forward().transpose(-1, -2)

    def network():
        xin = x.detach().requires_grad_(True)
        cls, _ = net(xin)
        torch.nn.functional.smooth_l1_loss(cls.reshape(B, T), f0).backward()
        return xin.grad

    def chain():
        w = wave.detach().requires_grad_(True)
        cls, _ = inference.f0_from_wave(net, w, mel_transform=mel, max_frames=T)
        torch.nn.functional.smooth_l1_loss(cls.reshape(B, T), f0).backward()
        return w.grad

    passes = {"mel_forward": mel_forward, "mel_backward": mel_backward, "network_fwd_input_grad_bwd": network,
              "chain_wave_to_loss_and_back": chain}
    ms = {k: [] for k in passes}
    for fn in passes.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize(dev)
    for _ in range(args.rounds):
        for name, fn in passes.items():
            ms[name].append(timed(fn, args.iters))
    dw = chain()
    assert bool(torch.isfinite(dw).all().item()) and bool(dw.any().item())
    assert not ops.persistent_lstm_error(dev)

    med = {k: statistics.median(v) for k, v in ms.items()}
    need = _lib.load().pe_mel_backward_workspace_bytes(mel._get_plan(dev), B, N, T)
    algo = B * valid * 4 * (2 * mel.hop_length + mel.n_mels)
    res = {"shape": {"batch": B, "samples": N, "frames": T, "valid_frames": valid},
           "device": torch.cuda.get_device_name(dev), "iters_per_round": args.iters,
           "passes": {k: {"ms": med[k], "rounds_ms": v} for k, v in ms.items()},
           "backward_over_forward": med["mel_backward"] / med["mel_forward"],
           "backward_share_of_chain": med["mel_backward"] / med["chain_wave_to_loss_and_back"],
           "backward_share_of_sum": med["mel_backward"] / (med["mel_forward"] + med["mel_backward"]
                                                           + med["network_fwd_input_grad_bwd"]),
           "mel_backward_bytes": {"algorithmic": algo, "algorithmic_TBps": algo / (med["mel_backward"] * 1e-3) / 1e12,
                                  "slab_workspace": need, "slab_written_and_read": 2 * need}}
    if args.kernel_stats:
        res["kernels"] = kernel_stats(args.kernel_stats)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
