"""The plain passes at the bottom of csrc/elementwise.hip (dropout, the strided copy, the sequence re-layouts, the
detector-tap max-pool, the segment absmax), attention's exported dropout mask and pe_colsum, off the one shape each
ran at.  Index, layout and stream work: everything here is bit for bit.

Every launcher below sizes its grid with ew_grid: at most 16384 blocks of 256 threads, one item (a float4 quad, or
an element for the re-layouts) per thread and pass.  A case that is meant to run a second grid pass asserts that its
item count exceeds EW_ITEMS_CAP.  pe_colsum and pe_absmax_segments have fixed grids (256 row chunks; 16 blocks per
segment) and loop inside them."""
import functools

import numpy as np
import pytest
import torch

from pitchextractor_amd import _lib, ops
from tests import small_ops_ref as S
from tests.test_ops_gpu import rnd

pytestmark = pytest.mark.gpu

EW_ITEMS_CAP = 16384 * 256
REFUSED = (ValueError, _lib.HipLibraryError)
DTYPES = [torch.float32, torch.bfloat16]


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == torch.bfloat16 else t.dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ dropout
DROP_SHAPES = [(1, 4), (3, 8), (257, 260), (4104, 4100)]
STREAMS = [(123, 0), (2 ** 63 + 5, 7), (5, 2 ** 32 - 3), (5, 2 ** 40 + 1)]
RATES = [0.0, 0.1, 0.5, 0.999]
# u == p exactly happens once in 2^24 draws, and only where float32(p) 2^24 is an integer (0, 0.5 and float32(0.999);
# not float32(0.1), a multiple of 2^-27): the (stream, p) pairs whose 4104 x 4100 draws hold such a tie -- where ">"
# instead of ">=" shows
TIES = [((123, 0), 0.0), ((123, 0), 0.999), ((5, 2 ** 32 - 3), 0.0), ((5, 2 ** 32 - 3), 0.999),
        ((5, 2 ** 40 + 1), 0.0), ((5, 2 ** 40 + 1), 0.5)]


@functools.lru_cache(maxsize=2)
def words(seed, offset, n_quads, rounds=10):
    return S.dropout_words(seed, offset, n_quads, rounds)


@functools.lru_cache(maxsize=4)
def drop_input(rows, cols):
    return rnd(rows, cols, seed=rows + cols)


def keep_on(dev, w, p, rows, cols, strict=False):
    return torch.from_numpy(S.keep_from_words(w, p, strict)).view(rows, cols).to(dev)


def dropped(x, keep, p):
    """x keep (1f / (1f - p)) in x's precision: dropped elements are +0."""
    y = x.float() * float(S.dropout_scale(p))
    return torch.where(keep.bool(), y, torch.zeros_like(y)).to(x.dtype)


def test_dropout_large_shape_crosses_the_grid_cap():
    rows, cols = DROP_SHAPES[-1]
    assert rows * (cols // 4) > EW_ITEMS_CAP
    assert all(r * (c // 4) <= EW_ITEMS_CAP for r, c in DROP_SHAPES[:-1])
    # the third stream's counters cross into the high word inside the two larger tensors
    assert 2 ** 32 - 3 + 257 * 65 > 2 ** 32


@pytest.mark.parametrize("seed,offset", STREAMS)
@pytest.mark.parametrize("rows,cols", DROP_SHAPES)
def test_dropout_is_the_philox_stream(hip_device, rows, cols, seed, offset):
    """Mask byte for byte and y bit for bit against dropout_keep_ref, at every rate; replaying the mask gives y again."""
    dev = hip_device
    xd = drop_input(rows, cols).to(dev)
    w = words(seed, offset, rows * cols // 4)
    for p in RATES:
        y, mask = ops.dropout(xd, p, seed=seed, offset=offset)
        keep = keep_on(dev, w, p, rows, cols)
        assert torch.equal(mask, keep), p
        assert same_bits(y, dropped(xd, keep, p)), p
        if p == 0.0:
            assert same_bits(y, xd) and bool(mask.all())
        y2, _ = ops.dropout(xd, p, mask_in=mask)
        assert same_bits(y2, y)
        if (rows, cols) == DROP_SHAPES[-1]:
            # controls: nine rounds draw another mask; ">" differs from ">=" exactly where a draw equals p
            w9 = words(seed, offset, rows * cols // 4, 9)
            assert torch.equal(mask, keep_on(dev, w9, p, rows, cols)) == (p == 0.0)      # p = 0 keeps whatever is drawn
            strict_differs = not torch.equal(mask, keep_on(dev, w, p, rows, cols, strict=True))
            assert strict_differs == (((seed, offset), p) in TIES), p


@pytest.mark.parametrize("k", [7, 2 ** 32 - 3, 2 ** 40 + 1])
def test_dropout_consecutive_calls_continue_the_stream(hip_device, k):
    """offset = k, then offset = k + rows cols / 4: the two masks, concatenated, are the reference stream of the whole
    range -- what _DropoutCfg.next_offset relies on, also across 2^32."""
    dev, rows, cols, seed = hip_device, 257, 260, 2 ** 63 + 5
    xd = drop_input(rows, cols).to(dev)
    nq = rows * cols // 4
    _, m1 = ops.dropout(xd, 0.5, seed=seed, offset=k)
    _, m2 = ops.dropout(xd, 0.5, seed=seed, offset=k + nq)
    both = torch.cat([m1.view(-1), m2.view(-1)]).cpu().numpy()
    assert np.array_equal(both, S.dropout_keep_ref(seed, k, 2 * nq, 0.5))
    assert not torch.equal(m1, m2)


@pytest.mark.parametrize("rows,cols", DROP_SHAPES[:3])
def test_dropout_bf16_and_strided(hip_device, rows, cols):
    dev, seed, offset, p = hip_device, 5, 2 ** 32 - 3, 0.1
    x = drop_input(rows, cols)
    keep = keep_on(dev, words(seed, offset, rows * cols // 4), p, rows, cols)
    # bf16 tensors: the same mask, y = bf16(x_f32 scale)
    xb = x.bfloat16().to(dev)
    yb, mb = ops.dropout(xb, p, seed=seed, offset=offset)
    assert torch.equal(mb, keep) and yb.dtype == torch.bfloat16 and same_bits(yb, dropped(xb, keep, p))
    # column slices of wider buffers (offsets multiples of 8 elements), NaN around the input, canaries around the output
    for dt in DTYPES:
        xbuf = torch.full((rows, cols + 24), float("nan"), dtype=dt, device=dev)
        xv = xbuf[:, 8:8 + cols]
        xv.copy_(x)
        obuf = torch.full((rows, cols + 16), -777.25, dtype=dt, device=dev)
        ov = obuf[:, 8:8 + cols]
        _, m = ops.dropout(xv, p, out2d=ov, seed=seed, offset=offset)
        want = torch.full((rows, cols + 16), -777.25, dtype=dt, device=dev)
        want[:, 8:8 + cols] = dropped(xv.contiguous(), keep, p)
        assert torch.equal(m, keep) and same_bits(obuf, want), dt


def test_dropout_refuses_what_it_cannot_run(hip_device):
    dev = hip_device
    with pytest.raises(REFUSED):
        ops.dropout(torch.zeros(3, 8, device=dev), 1.0)
    with pytest.raises(REFUSED):
        ops.dropout(torch.zeros(3, 8, device=dev), -0.1)
    with pytest.raises(REFUSED):
        ops.dropout(torch.zeros(3, 6, device=dev), 0.5)
    with pytest.raises(REFUSED):
        ops.dropout(torch.zeros(3, 8, device=dev), 0.5, out2d=torch.zeros(3, 8, dtype=torch.bfloat16, device=dev))


# ------------------------------------------------------------------ attention's dropout mask
def test_attention_exports_the_dropout_stream(hip_device):
    """The keep bytes ops.attn_fwd exports are dropout_keep_ref under attention.hip's mapping: quad = row (T / 4) +
    col / 4 over the dense [B H T][T] probabilities.  Run at the smallest T the fused kernel supports and at one more
    if it supports another (the LayerNorm / GELU fused dropouts are tied to ops.dropout by the Transformer tests)."""
    dev, dh, B, H = hip_device, 64, 1, 2
    supported = [T for T in range(4, 1025, 4) if ops.attn_supported(T, dh)]
    assert supported, "the fused attention kernel supports no T"
    for T in sorted({supported[0], supported[-1]}):
        qkv = rnd(B * T, 3 * H * dh, seed=T).to(dev)
        for p, seed, offset in ((0.1, 2 ** 63 + 5, 7), (0.5, 5, 2 ** 32 - 100)):
            _, _, mask = ops.attn_fwd(qkv, B, T, H, dh ** -0.5, p, seed=seed, offset=offset)
            ref = S.dropout_keep_ref(seed, offset, B * H * T * T // 4, p).reshape(B * H * T, T)
            assert np.array_equal(mask.cpu().numpy(), ref), (T, p)
            assert not np.array_equal(ref, S.dropout_keep_ref(seed, offset, B * H * T * T // 4, p, rounds=9)
                                      .reshape(B * H * T, T))


# ------------------------------------------------------------------ copy2d
def sliced(t, pad, dev, fill=-777.25):
    """(buffer, view): t inside a buffer `pad` columns wider (pad = 0: t itself), 8 columns in."""
    if pad == 0:
        buf = t.to(dev).clone()
        return buf, buf
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=dev)
    view = buf[:, 8:8 + t.shape[1]]
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", DROP_SHAPES)
def test_copy2d(hip_device, rows, cols, dtype):
    """Dense / sliced sources and destinations with different row strides: a plain copy is bit-exact, accumulate is one
    add (fp32: dst + src; bf16: bf16(dst_f32 + src_f32)), bytes outside the destination slice keep their bits."""
    dev = hip_device
    if (rows, cols) == DROP_SHAPES[-1]:
        assert rows * (cols // 4) > EW_ITEMS_CAP
    src, dst = rnd(rows, cols, seed=1).to(dtype), rnd(rows, cols, seed=2).to(dtype)
    for spad, dpad in ((0, 0), (16, 0), (0, 24), (16, 24)):
        for acc in (False, True):
            sbuf, sv = sliced(src, spad, dev, fill=float("nan"))
            dbuf, dv = sliced(dst, dpad, dev)
            want = dbuf.clone()
            wv = want[:, 8:8 + cols] if dpad else want
            wv.copy_((dv.float() + sv.float()).to(dtype) if acc else sv)
            keep_src = bits(sbuf).clone()
            out = ops.copy2d(sv, dv, accumulate=acc)
            assert out is dv and same_bits(dbuf, want), (spad, dpad, acc)
            assert torch.equal(bits(sbuf), keep_src)


def test_copy2d_refuses_what_it_cannot_run(hip_device):
    dev = hip_device
    with pytest.raises(REFUSED):
        ops.copy2d(torch.zeros(3, 8, device=dev), torch.zeros(3, 8, dtype=torch.bfloat16, device=dev))
    with pytest.raises(REFUSED):
        ops.copy2d(torch.zeros(3, 6, device=dev), torch.zeros(3, 6, device=dev))
    with pytest.raises(REFUSED):
        ops.copy2d(torch.zeros(3, 8, device=dev), torch.zeros(4, 8, device=dev))


# ------------------------------------------------------------------ (B, C, T, 2) <-> (B, T, 2 C)
SEQ_LAYOUTS = [(1, 1), (2, 7), (4, 4100)]                      # (B, T): B T = 1, 14, 16400


def seq_cases():
    for C in (1, 3, 64, 256):
        for ld, coff in ((640, 0), (640, 64), (640, 384), (C, 0)):
            for B, T in SEQ_LAYOUTS:
                if B * T == 16400 and not (C == 256 and coff in (384, 0)):
                    continue                                    # the large row count only where it crosses the cap
                yield C, ld, coff, B, T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,ld,coff,B,T", list(seq_cases()))
def test_seq_relayouts(hip_device, C, ld, coff, B, T, dtype):
    """seq[b, t, c 2 + w] = x[b, t, w, coff + c]: bit-exact both ways (the permute of test_seq_relayout); accumulate is
    one add in the destination's precision; channels outside [coff, coff + C) keep their bits."""
    dev = hip_device
    if B * T == 16400:
        assert B * T * C > EW_ITEMS_CAP
    x = rnd(B, T, 2, ld, seed=C + coff).to(dtype).to(dev)
    ref = x[..., coff:coff + C].float().permute(0, 1, 3, 2).reshape(B, T, 2 * C)
    seq = ops.nhwc_to_seq(x, C, coff=coff)
    assert seq.dtype == torch.float32 and same_bits(seq, ref.contiguous())
    # back into a pre-filled tensor
    seq_in = rnd(B, T, 2 * C, seed=7).to(dev)
    base = rnd(B, T, 2, ld, seed=8).to(dtype).to(dev)
    val = seq_in.view(B, T, C, 2).permute(0, 1, 3, 2)
    out = base.clone()
    ops.seq_to_nhwc(seq_in, out, C, coff=coff)
    want = base.clone()
    want[..., coff:coff + C] = val.to(dtype)
    assert same_bits(out, want)
    ops.seq_to_nhwc(seq_in, out, C, coff=coff, accumulate=True)
    want2 = want.clone()
    want2[..., coff:coff + C] = (want[..., coff:coff + C].float() + val).to(dtype)
    assert same_bits(out, want2)
    if dtype == torch.float32:
        assert same_bits(out[..., coff:coff + C], 2 * want[..., coff:coff + C])          # fp32: it doubles


# ------------------------------------------------------------------ plain max-pool (detector taps)
POOLS = [1, 2, 3, 4, 5, 7, 8, 9, 10, 16]


def pool_input(B, T, Fq, C, dtype, ties, seed):
    """Continuous values, or integers in [-2, 2] full of ties with +0.0 and -0.0 mixed."""
    g = torch.Generator().manual_seed(seed)
    if not ties:
        return torch.randn(B, T, Fq, C, generator=g).to(dtype)
    x = torch.randint(-2, 3, (B, T, Fq, C), generator=g).float()
    x[torch.rand(B, T, Fq, C, generator=g) < 0.25] *= -1.0       # zeros become -0.0
    return x.to(dtype)


def pool_check(dev, x, pool, coff=8, pad=16, seed=0, last_misses=False):
    """Forward values and positions, then the backward from a random pre-filled dx through both paths."""
    B, T, Fq, C = x.shape
    dtype, Fo = x.dtype, Fq // pool
    val, pos = S.maxpool_ref(x.float().numpy(), pool)
    xd = x.to(dev)
    wide = torch.full((B, T, Fo, C + pad), -777.25, dtype=dtype, device=dev)
    out, arg = ops.maxpool_fwd(xd, pool, out=wide, coff=coff, want_argmax=True)
    want = torch.full((B, T, Fo, C + pad), -777.25, dtype=dtype, device=dev)
    want[..., coff:coff + C] = torch.from_numpy(val).to(dtype).to(dev)
    assert same_bits(wide, want)
    assert arg.dtype == torch.uint8 and np.array_equal(arg.cpu().numpy(), pos)
    wide2 = torch.full((B, T, Fo, C + pad), -777.25, dtype=dtype, device=dev)
    ops.maxpool_fwd(xd, pool, out=wide2, coff=coff)
    assert same_bits(wide2, want)
    if last_misses:
        assert not np.array_equal(arg.cpu().numpy(), S.maxpool_ref(x.float().numpy(), pool, last=True)[1])
    # backward: one add per window and channel at the first maximum; the remainder of F keeps its bits
    g = torch.Generator().manual_seed(seed + 1)
    dy = torch.randn(B, T, Fo, C + pad, generator=g).to(dtype)
    base = torch.randn(B, T, Fq, C, generator=g).to(dtype)
    exp = base.float().numpy().copy()
    win = exp[:, :, :Fo * pool].reshape(B, T, Fo, pool, C)
    idx = pos.astype(np.int64)[..., None, :]
    upd = np.take_along_axis(win, idx, axis=3) + dy[..., coff:coff + C].float().numpy()[..., None, :]
    np.put_along_axis(win, idx, upd, axis=3)
    exp[:, :, :Fo * pool] = win.reshape(B, T, Fo * pool, C)
    want_dx = torch.from_numpy(exp).to(dtype).to(dev)
    dyd = dy.to(dev)
    dx1, dx2 = base.to(dev), base.to(dev)
    ops.maxpool_bwd_add(xd, dyd, dx1, pool, coff=coff)
    ops.maxpool_bwd_add(xd, dyd, dx2, pool, coff=coff, argmax=arg)
    assert same_bits(dx1, want_dx) and same_bits(dx2, dx1)
    if Fo * pool < Fq:
        assert same_bits(dx1[:, :, Fo * pool:], base[:, :, Fo * pool:].to(dev))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pool", POOLS)
def test_maxpool_against_first_maximum(hip_device, pool, dtype):
    """pool 1 .. 16: the four-rows-in-flight loop leaves remainders 0 .. 3; F = pool, 2 pool + 1 (a remainder the pool
    ignores) and 23; C = 4, 64, 260; into a channel slice of a wider tensor."""
    assert {(p - 1) % 4 for p in POOLS} == {0, 1, 2, 3}
    for Fq in sorted({pool, 2 * pool + 1, 23}):
        for C in (4, 64, 260):
            for ties in (False, True):
                x = pool_input(2, 3, Fq, C, dtype, ties, seed=pool * 1000 + Fq + C)
                pool_check(hip_device, x, pool, seed=Fq + C, last_misses=ties and pool > 1 and C >= 64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool_window_wider_than_the_rows_writes_nothing(hip_device, dtype):
    dev, pool = hip_device, 5
    x = pool_input(2, 3, 4, 8, dtype, False, seed=1).to(dev)
    wide = torch.empty((2, 3, 0, 24), dtype=dtype, device=dev)
    out, arg = ops.maxpool_fwd(x, pool, out=wide, coff=8, want_argmax=True)
    assert out.numel() == 0 and arg.shape == (2, 3, 0, 8)
    assert ops.maxpool_fwd(x, pool).shape == (2, 3, 0, 8)
    dx = pool_input(2, 3, 4, 8, dtype, False, seed=2).to(dev)
    keep = dx.clone()
    ops.maxpool_bwd_add(x, wide, dx, pool, coff=8)
    ops.maxpool_bwd_add(x, wide, dx, pool, coff=8, argmax=arg)
    assert same_bits(dx, keep)


def test_maxpool_second_grid_pass(hip_device):
    """The smallest pool-2 size whose (window, channel quad) count exceeds the cap: 16385 x 16 windows of 16 quads,
    with a remainder row (F = 33).  Tie-laden input, so positions are at stake in both passes."""
    B, T, Fq, C, pool = 1, 16385, 33, 64, 2
    n_items = B * T * (Fq // pool) * (C // 4)
    assert n_items > EW_ITEMS_CAP and (B * T - 1) * (Fq // pool) * (C // 4) <= EW_ITEMS_CAP
    pool_check(hip_device, pool_input(B, T, Fq, C, torch.float32, True, seed=3), pool, last_misses=True)


def test_maxpool_refuses_a_position_that_does_not_fit_a_byte(hip_device):
    dev = hip_device
    x = torch.zeros(1, 1, 256, 4, device=dev)
    with pytest.raises(REFUSED):
        ops.maxpool_fwd(x, 256, want_argmax=True)
    with pytest.raises(REFUSED):
        ops.maxpool_fwd(torch.zeros(1, 1, 4, 6, device=dev), 2)


# ------------------------------------------------------------------ column sums
@pytest.mark.parametrize("rows", [1, 2, 3, 5, 17, 255, 256, 257, 4099])
def test_colsum_is_the_rounded_double_sum(hip_device, rows):
    """+-1e6 plus unit noise: the columns cancel to a few units.  pe_colsum accumulates in double, so only the last
    rounding may differ from float32(sum in float64): 1 ulp.  (Every element is a multiple of 2^-4 below 2^20, so the
    double sums are in fact exact.)  Dense and as a column slice with ld > cols; out1 is out0's bits."""
    dev = hip_device
    for cols in (4, 8, 252, 260, 1536):
        sign = torch.where(torch.arange(rows)[:, None] % 2 == 0, 1.0, -1.0)
        x = (sign * 1e6 + rnd(rows, cols, seed=rows + cols))
        ref = x.double().sum(0).numpy()
        ref32 = ref.astype(np.float32)
        assert rows % 2 == 1 or np.abs(ref).max() < 1e3
        buf = torch.full((rows, cols + 24), float("nan"), device=dev)
        view = buf[:, 8:8 + cols]
        view.copy_(x)
        for src in (x.to(dev), view):
            a, b = torch.full((cols,), float("nan"), device=dev), torch.full((cols,), float("nan"), device=dev)
            ops.colsum(src, a, b)
            got = a.cpu().numpy()
            assert (np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref32)).astype(np.float64)).all(), cols
            assert same_bits(a, b)
            c = torch.full((cols,), float("nan"), device=dev)
            ops.colsum(src, c)
            assert same_bits(c, a)


# ------------------------------------------------------------------ absmax of segments
SEG_LENS = [0, 1, 3, 4096, 4097, 5000]


def seg_ref(flat, off, length):
    b = flat.numpy().view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.array([b[o:o + n].max() if n else 0 for o, n in zip(off, length)], dtype=np.uint32)


@pytest.mark.parametrize("nseg", [1, 300])
def test_absmax_segments(hip_device, nseg):
    """Exact bits of max |x| per segment: odd, unaligned offsets; the maximum planted at each segment's last element; a
    zero-length segment leaves 0; a segment holding a NaN gives the NaN's magnitude bits."""
    dev = hip_device
    rounds = [[n] for n in SEG_LENS] if nseg == 1 else [[SEG_LENS[i % len(SEG_LENS)] for i in range(nseg)]]
    for lens in rounds:
        off, pos = [], 1
        for n in lens:
            off.append(pos)
            pos += n + (2 if n % 2 == 0 else 1)                     # gaps keep every offset odd
        flat = rnd(pos + 8, seed=len(lens) + lens[0])
        for i, (o, n) in enumerate(zip(off, lens)):
            if n:
                flat[o + n - 1] = -(10.0 + i)                        # the last element holds the maximum
                flat[o + n] = 1e6                                    # and the one after it is not the segment's
        assert all(o % 2 == 1 for o in off)
        seg_off = torch.tensor(off, dtype=torch.int64, device=dev)
        seg_len = torch.tensor(lens, dtype=torch.int64, device=dev)
        out = torch.full((len(lens),), -1, dtype=torch.int32, device=dev)
        got = ops.absmax_segments(flat.to(dev), seg_off, seg_len, out=out).cpu().numpy().view(np.uint32)
        ref = seg_ref(flat, off, lens)
        assert np.array_equal(got, ref)
        for i, n in enumerate(lens):
            assert got[i] == (np.float32(10.0 + i).view(np.uint32) if n else 0)
        # a NaN inside the largest segment
        big = int(np.argmax(lens))
        if lens[big] > 1:
            flat[off[big] + lens[big] // 2] = float("nan")
            got = ops.absmax_segments(flat.to(dev), seg_off, seg_len).cpu().numpy().view(np.uint32)
            assert np.array_equal(got, seg_ref(flat, off, lens)) and got[big] == 0x7FC00000
