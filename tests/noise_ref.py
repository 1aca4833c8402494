"""Float64 restatement of the additive-noise path (``csrc/noise.hip`` through ``pitchextractor_amd.noise``): the seeded
standard normals, the colour recurrence run sample by sample, the looped bed and the mix at an SNR with every float32
rounding in its stated place.  Nothing here knows about pieces, scans or layouts.

Conventions: Philox4x32-10 as ``csrc/common.h`` states it (key = the two halves of the seed, counter = ``{lo, hi, 0,
0}`` of the sample index); ``u1 = ((w0 >> 8) + 0.5) 2^-24``, ``u2 = (w1 >> 8) 2^-24``, ``z = sqrt(-2 ln u1) cos(2 pi
u2)``; sample ``i`` of a row is generated sample ``warmup + i``; the SNR is over the whole row, silence included; a row
of length 0 yields nothing and its stats are ``{0, 0, 0, 0}``."""
import numpy as np

PIECE = 2048
MAX_SECTIONS = 8
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
PINK = (0.5362, 0.115926, ((0.99886, 0.0555179), (0.99332, 0.0750759), (0.96900, 0.1538520), (0.86650, 0.3104856),
                           (0.55000, 0.5329522), (-0.7616, -0.0168980)))


def philox4x32(seed: int, counters, rounds: int = 10) -> np.ndarray:
    """The four 32-bit words of Philox4x32-10 for every counter: ``(len(counters), 4)`` uint32.  (``rounds``: another
    round count, for controls that must miss.)"""
    ctr = np.asarray(counters, dtype=np.uint64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = [ctr & MASK, ctr >> np.uint64(32), np.zeros_like(ctr), np.zeros_like(ctr)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]                       # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def uniforms(seed: int, counters):
    """``(u1, u2)`` in float64, exact: ``u1`` has 25 significant bits (float32 rounds it), ``u2`` has 24."""
    w = philox4x32(seed, counters).astype(np.uint64)
    return ((w[:, 0] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24, \
        (w[:, 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def randn64(seed: int, counters) -> np.ndarray:
    """Box-Muller of the two words in float64."""
    u1, u2 = uniforms(seed, counters)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def randn32_numpy(seed: int, counters) -> np.ndarray:
    """The same expression evaluated by numpy in float32 throughout, the sum ``(w0 >> 8) + 0.5`` included."""
    w = philox4x32(seed, counters)
    f = np.float32
    u1 = ((w[:, 0] >> np.uint32(8)).astype(f) + f(0.5)) * f(2.0 ** -24)
    u2 = (w[:, 1] >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    out = np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(2.0) * f(np.pi) * u2)
    assert out.dtype == f
    return out


def white(n: int, seed: int, warmup: int = 0) -> np.ndarray:
    """Float64 standard normals of generated samples ``warmup .. warmup + n``."""
    return randn64(seed, np.arange(warmup, warmup + n, dtype=np.uint64))


def colour(w, d0, d1, sections, warmup: int = 0) -> np.ndarray:
    """``y[j] = d0 w[j] + d1 w[j - 1] + sum_k s_k[j]``, ``s_k[j] = a_k s_k[j - 1] + b_k w[j]`` from zero, in double,
    sample by sample and section by section in order; the samples from ``warmup`` on, rounded once to float32."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    state = [0.0] * len(sections)
    out = np.zeros(w.size, np.float64)
    before = 0.0
    for j, v in enumerate(w.tolist()):
        acc = d0 * v + d1 * before
        for k, (a, b) in enumerate(sections):
            state[k] = a * state[k] + b * v
            acc += state[k]
        out[j] = acc
        before = v
    return out[warmup:].astype(np.float32)


def lfilter_form(d0, d1, sections):
    """``(b, a)`` lists, one pair per parallel branch, for ``scipy.signal.lfilter``: the direct taps and every
    section."""
    return [([d0, d1], [1.0])] + [([b], [1.0, -a]) for a, b in sections]


def response_db(d0, d1, sections, freqs_hz, sr) -> np.ndarray:
    """The analytic magnitude response of the colour in dB at ``freqs_hz``."""
    z1 = np.exp(-2j * np.pi * np.asarray(freqs_hz, np.float64) / sr)
    h = d0 + d1 * z1
    for a, b in sections:
        h = h + b / (1.0 - a * z1)
    return 20.0 * np.log10(np.abs(h))


def bed(recording, n: int, start: int) -> np.ndarray:
    """``out[i] = bed[(start + i) mod L]``."""
    recording = np.asarray(recording, dtype=np.float32).reshape(-1)
    return recording[(int(start) + np.arange(n)) % recording.size]


def rms(x) -> float:
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return float(np.sqrt(np.sum(x * x) / x.size)) if x.size else 0.0


def mix(x, noise, snr_db, peak_normalize: bool = True, scale=None):
    """``(y, stats)`` of the mix: ``stats = {peak, rms_signal, rms_noise, scale}``.  ``scale``: use this float32 scale
    instead of the one computed here (the device's own, to compare ``y`` bit for bit)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    noise = np.asarray(noise, dtype=np.float32).reshape(-1)
    if x.size == 0:
        return x.copy(), np.zeros(4)
    rs, rn = rms(x), rms(noise)
    if scale is None:
        scale = np.float32((rs / 10.0 ** (float(snr_db) / 20.0)) / rn) if rs > 0.0 and rn > 0.0 else np.float32(0.0)
    scale = np.float32(scale)
    y = x.copy() if scale == 0 else (x + (noise * scale).astype(np.float32)).astype(np.float32)
    peak = float(np.max(np.abs(y)))
    if peak_normalize and peak > 0.99:
        y = (y / np.float32(peak + 1e-6)).astype(np.float32)
    return y, np.array([peak, rs, rn, float(scale)])


def summarize_with_drop(records, baseline_records, group_keys, metrics=("RPA", "RCA", "VUV", "OctaveError")):
    """The notebooks' summary-with-drop table, restated with plain loops: per group (in order of first appearance) the
    NaN-skipping mean and sample std (ddof 1; NaN below two values) of every metric, and its drop against the baseline's
    NaN-skipping mean: baseline - mean for the metrics where higher is better, mean - baseline for ``OctaveError``."""
    def clean(rows, key):
        return [float(r[key]) for r in rows if not np.isnan(float(r[key]))]

    def mean(vals):
        return sum(vals) / len(vals) if vals else float("nan")

    groups = {}
    for rec in records:
        groups.setdefault(tuple(rec[k] for k in group_keys), []).append(rec)
    table = []
    for key, rows in groups.items():
        line = dict(zip(group_keys, key))
        for metric in metrics:
            vals = clean(rows, metric)
            m = mean(vals)
            line[metric + "_mean"] = m
            line[metric + "_std"] = (float(np.sqrt(sum((v - m) ** 2 for v in vals) / (len(vals) - 1)))
                                     if len(vals) >= 2 else float("nan"))
        for metric in metrics:
            base = mean(clean(baseline_records, metric))
            line[metric + "_drop"] = line[metric + "_mean"] - base if metric == "OctaveError" \
                else base - line[metric + "_mean"]
        table.append(line)
    return table
