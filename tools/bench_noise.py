"""Device cost of additive noise at an SNR (pitchextractor_amd.noise) next to the inference it feeds and to the host.

Two batches at 24 kHz: 64 rows of 4 s, and one 5-minute row beside 63 rows of 2 s.  Per batch and per call, host work
included (the row plan, its upload, the output allocation), between two device events after a warm-up: drawn white,
pink and brown noise, a looped 10 s bed, the mix at 10 dB, and ``stress.apply_additive_noise`` with pink noise.  Next to
them, in the same session: ``predict_f0_batch`` on the same rows (a randomly initialised default JDCNet), and the same
pink noise built on the host (``numpy`` standard normals through ``scipy.signal.lfilter``, one branch per section,
the warm-up included) and uploaded.  Per stage also the entry point alone in a loop on a prepared plan (``kernel_ms``:
the launches queue back to back, so this is device time), the bytes it moves computed from the shapes, and that rate as
a share of the device-to-device copy rate measured here.  Writes profiles/bench_noise.json and prints the JSON line.
Needs a GPU; there is no fallback.

Not a gate: the statement to support is what share of a noise sweep the noise costs next to the model's forward, and
what the device path saves over building the noise on the host.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import _lib, inference, noise as N, ops, stress  # noqa: E402
from pitchextractor_amd.model import JDCNet  # noqa: E402

SR = 24000
WARMUP = 4096


def timed_loop(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def timed(fn):
    fn()
    torch.cuda.synchronize()
    first = timed_loop(fn, 1)
    return timed_loop(fn, max(2, min(50, int(300.0 / max(first, 1e-3)))))


def copy_rate(dev):
    """bytes/s (read + write) of a device-to-device copy of 256 MiB."""
    src = torch.empty((64 << 20,), dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        dst.copy_(src)
    b.record()
    b.synchronize()
    return 2.0 * src.numel() * 4 * 10 / (a.elapsed_time(b) * 1e-3)


def host_pink(lengths, dev):
    """Pink noise of every row on the host (numpy + scipy.signal.lfilter, warm-up included) and one upload: seconds."""
    from scipy.signal import lfilter
    d0, d1, sections = N.colour_sections("pink", SR)
    t0 = time.perf_counter()
    rows = []
    for r, n in enumerate(lengths):
        w = np.random.default_rng(r).standard_normal(n + WARMUP)
        y = lfilter([d0, d1], [1.0], w)
        for a, b in sections:
            y = y + lfilter([b], [1.0, -a], w)
        rows.append(y[WARMUP:].astype(np.float32))
    torch.from_numpy(np.concatenate(rows)).to(dev)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_stages(lengths, x, noise, beds, dev):
    """ms per call of each entry point alone on a prepared plan, and the bytes it moves."""
    n = int(sum(lengths))
    stream = _lib.stream_ptr()
    out = {}
    y = torch.empty((n,), dtype=torch.float32, device=dev)

    def stage(name, moved, fn):
        ms = timed(fn)
        out[name] = {"kernel_ms": ms, "bytes": moved, "bytes_per_s": moved / (ms * 1e-3)}

    pl = N.to_device(N.plan_rows(lengths), dev)
    stage("white", 4 * n, lambda: ops._call("pe_noise_white", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data,
                                             pl["rows"], y.data_ptr(), stream))
    for colour in ("pink", "brown"):
        pc = N.to_device(N.plan_rows(lengths, warmup=WARMUP, colour=colour, sr=SR), dev)
        n_bytes = _lib.load().pe_noise_workspace_bytes(pc["n_pieces"])
        ws = torch.empty((max(n_bytes, 1),), dtype=torch.uint8, device=dev)
        # the samples written, and the piece states written, read, rewritten and read
        stage(colour, 4 * n + 4 * n_bytes,
              lambda pc=pc, ws=ws, n_bytes=n_bytes: ops._call(
                  "pe_noise_colour", pc["meta_d"].data_ptr(), pc["meta"].ctypes.data, pc["params_d"].data_ptr(),
                  pc["params"].ctypes.data, 0, 0, pc["rows"], y.data_ptr(), ws.data_ptr(), n_bytes, stream))
    table = np.zeros((len(lengths), pl["bed_fields"]), np.int64)
    table[:, 1] = beds.lengths[0]
    table_d = torch.from_numpy(table).to(dev)
    audio = beds.audio(dev)
    stage("bed", 8 * n, lambda: ops._call("pe_noise_bed", pl["meta_d"].data_ptr(), pl["meta"].ctypes.data,
                                           audio.data_ptr(), audio.numel(), table_d.data_ptr(), table.ctypes.data,
                                           pl["rows"], y.data_ptr(), stream))
    snr = np.full(len(lengths), 10.0)
    snr_d = torch.from_numpy(snr).to(dev)
    stats = torch.zeros((len(lengths), pl["stat_fields"]), dtype=torch.float64, device=dev)
    n_bytes = _lib.load().pe_noise_workspace_bytes(pl["n_pieces"])
    ws = torch.empty((max(n_bytes, 1),), dtype=torch.uint8, device=dev)
    # sums read x and noise, the mix reads them again and writes y (the peak rule does not fire at this level)
    stage("mix", 20 * n, lambda: ops._call("pe_noise_mix", x.data_ptr(), noise.data_ptr(), pl["meta_d"].data_ptr(),
                                            pl["meta"].ctypes.data, snr_d.data_ptr(), snr.ctypes.data, 1, pl["rows"],
                                            y.data_ptr(), stats.data_ptr(), ws.data_ptr(), n_bytes, stream))
    return out


def bench_set(name, lengths, net, beds, dev, rate):
    n = int(sum(lengths))
    t = torch.arange(n, dtype=torch.float32, device=dev)
    x = (0.1 * torch.sin(t * (2.0 * np.pi * 220.0 / SR))).contiguous()
    res = {"rows": len(lengths), "samples": n, "ms": {}}
    res["ms"]["white"] = timed(lambda: N.white(lengths, 0, dev))
    res["ms"]["pink"] = timed(lambda: N.coloured(lengths, "pink", SR, seeds=0, warmup=WARMUP, device=dev))
    res["ms"]["brown"] = timed(lambda: N.coloured(lengths, "brown", SR, seeds=0, warmup=WARMUP, device=dev))
    res["ms"]["bed"] = timed(lambda: N.bed(beds, lengths, 0, 0, device=dev))
    noise = N.coloured(lengths, "pink", SR, seeds=0, warmup=WARMUP, device=dev)
    res["ms"]["mix"] = timed(lambda: N.mix_at_snr(x, noise, 10.0, lengths))
    res["ms"]["apply_additive_noise_pink"] = timed(lambda: stress.apply_additive_noise(x, SR, 10.0, "pink",
                                                                                       lengths=lengths))
    predict = lambda: inference.predict_f0_batch(net, x, lengths, stitch="concat")  # noqa: E731
    predict()
    torch.cuda.synchronize()
    res["ms"]["predict_f0_batch"] = timed_loop(predict, 2)
    res["ms"]["host_pink_numpy_scipy_plus_upload"] = host_pink(lengths, dev) * 1e3
    res["noise_share_of_sweep"] = res["ms"]["apply_additive_noise_pink"] / (res["ms"]["apply_additive_noise_pink"]
                                                                            + res["ms"]["predict_f0_batch"])
    res["stages"] = kernel_stages(lengths, x, noise, beds, dev)
    for st in res["stages"].values():
        st["share_of_copy_rate"] = st["bytes_per_s"] / rate
    print(f"[bench_noise] {name}: {json.dumps(res)}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_noise.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = JDCNet(num_class=1).to(dev).eval()
    beds = N.NoiseSet([np.random.default_rng(1).standard_normal(10 * SR).astype(np.float32)], dev)
    rate = copy_rate(dev)
    res = {"sr": SR, "warmup": WARMUP, "copy_bytes_per_s": rate, "sets": {}}
    res["sets"]["64_rows_of_4s"] = bench_set("64 x 4 s", [4 * SR] * 64, net, beds, dev, rate)
    res["sets"]["5min_row_and_63_of_2s"] = bench_set("5 min + 63 x 2 s", [300 * SR] + [2 * SR] * 63, net, beds, dev,
                                                      rate)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
