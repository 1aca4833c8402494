"""Test helper: the mel parameter sets of the off-default tests, and a pure-Python restatement of how
``pe_mel_plan_create`` (csrc/mel.hip) cuts the sparse filterbank into 8-tap chunks.

The chunk table is computed from the ORACLE filterbank (oracle/mel_ref.mel_filterbank) rounded to float32, not
from the library, so that the CPU suite can pin which edges of the plan each GPU parameter set reaches:
a filter of exactly ``MAX_CHUNKS`` chunks, an empty filter, ``n_mels > 64``, a pair count near ``MAX_PAIRS``.
"""
import numpy as np

from oracle import mel_ref

TAPS = 8            # bins per chunk
MAX_CHUNKS = 6      # kMaxParts in csrc/mel.hip
MAX_PAIRS = 256     # chunk sums of one frame live in a 256-float region

# (id, MelSpectrogram keywords, (n_pairs, max chunks per filter, empty filters)); the last two sets keep the default
# filterbank and change only the hop
PARAM_SETS = [
    ("sr16k", dict(sample_rate=16000, hop_length=160, n_mels=80), (159, 5, 0)),
    ("mels128", dict(sample_rate=24000, hop_length=256, n_mels=128), (191, 3, 0)),
    ("sr44k1_hop441", dict(sample_rate=44100, hop_length=441, n_mels=80), (163, 6, 0)),
    ("sr22k05_hop275", dict(sample_rate=22050, hop_length=275, n_mels=64), (153, 6, 0)),
    ("band50_7600", dict(sample_rate=24000, hop_length=300, n_mels=80, f_min=50.0, f_max=7600.0), (116, 3, 0)),
    ("band0_4000", dict(sample_rate=24000, hop_length=300, n_mels=80, f_min=0.0, f_max=4000.0), (84, 2, 0)),
    ("mels200", dict(sample_rate=24000, hop_length=300, n_mels=200), (240, 2, 1)),
    ("hop75", dict(sample_rate=24000, hop_length=75, n_mels=80), (162, 5, 0)),
    ("hop1200", dict(sample_rate=24000, hop_length=1200, n_mels=80), (162, 5, 0)),
]
PARAM_IDS = [p[0] for p in PARAM_SETS]

# parameter sets the plan must refuse: (id, keywords, (n_pairs, max chunks, empty filters))
REJECTED_SETS = [
    ("mels40", dict(sample_rate=24000, hop_length=300, n_mels=40), (139, 9, 0)),
    ("mels256", dict(sample_rate=24000, hop_length=300, n_mels=256), (280, 2, 7)),
]


def mel_kwargs(params: dict) -> dict:
    """Full keyword set (n_fft = win_length = 1024) for MelSpectrogram and the oracle alike."""
    return dict(n_fft=1024, win_length=1024, **params)


def filterbank32(sample_rate=24000, n_mels=80, f_min=0.0, f_max=None, n_fft=1024, **_unused) -> np.ndarray:
    """(n_freqs, n_mels) oracle filterbank rounded to float32, the precision the plan stores."""
    f_max = float(sample_rate // 2) if f_max is None else float(f_max)
    return mel_ref.mel_filterbank(n_fft // 2 + 1, float(f_min), f_max, n_mels, sample_rate).astype(np.float32)


def filter_extents(fb32: np.ndarray):
    """Per filter (first, last) non-zero bin, or (-1, -1) for a filter without one."""
    out = []
    for col in fb32.T:
        nz = np.flatnonzero(col != 0.0)
        out.append((int(nz[0]), int(nz[-1])) if nz.size else (-1, -1))
    return out


def chunk_table(**params):
    """(n_pairs, max_chunks, n_empty): total 8-tap chunks, the most one filter needs, filters with no bin."""
    chunks = []
    for first, last in filter_extents(filterbank32(**params)):
        length = 0 if first < 0 else last - first + 1
        chunks.append(-(-length // TAPS))
    return sum(chunks), max(chunks), sum(1 for c in chunks if c == 0)


def empty_filters(**params):
    return [m for m, (first, _) in enumerate(filter_extents(filterbank32(**params))) if first < 0]
