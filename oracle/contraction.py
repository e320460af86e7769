"""CPU bit-model of the three contraction schemes of the fused conv kernels (tqdne_amd/csrc/conv1d_kernel.hpp, SCH 0 / 1 / 2) and of
the packed-weight layouts of tq_pack_conv_weight (tqdne_amd/csrc/conv1d_mfma.hip).  numpy only; every operand is rounded exactly as
the kernels round it, every product is exact and the sums run in float64 -- what remains between this model and a kernel is the fp32
accumulation order of the matrix cores (and, for GN + SiLU launches, the kernel's own exp / rcp).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Operand conventions.  A *block* is 16 consecutive channels of one row (activations: one position; weights: one output row) of one
tap; the fp16-range schemes carry the first-order corrections of a block as the element pairs {x_l * 2^12, x} on the activation side
and {W, W_l * 2^12} on the weight side, x_l = x - fp16(x), W_l = W - fp16(W):
  scheme 0 (bf16x3)    y = xh wh + xh wl + xl wh;  weights: hi = bf16(W), lo = bf16(W - hi), both round-to-nearest-even (split_bf16,
                       common.hpp); activations: hi = x TRUNCATED to bf16, lo = bf16(x - hi) rounded (write_one)
  scheme 1 (f16 + mx8) y = fp16(x) fp16(W) + 2^-12 [e4m3(x_l 2^12) e4m3(W) + e4m3(x) e4m3(W_l 2^12)], operands clamped to +-448 (x_l to
                       +-0.109375) before the conversion, uniform scales 2^0 / 2^-12
  scheme 2 (f16 + mx6) as 1 with e2m3 codes and one E8M0 scale per block and side: 2^e is the smallest power of two with
                       max(block) / 2^e <= 7.5 (e8m0_block_scale, conv_args.hpp), the activation side's byte carries the 2^-12
"""

from __future__ import annotations

import numpy as np

BF16X3, F16_MX8, F16_MX6 = 0, 1, 2      # TQ_WFMT_* of include/tqdne_hip.h
SCHEMES = (BF16X3, F16_MX8, F16_MX6)
SCHEME_NAME = {BF16X3: "bf16x3", F16_MX8: "f16+mx8", F16_MX6: "f16+mx6"}
E8M0_MIN, E8M0_MAX = 13, 254


def _f32(v):
    return np.ascontiguousarray(v, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ rounders
def bf16_rne_bits(v):
    """upper 16 bits of fp32 v rounded to nearest-even (finite inputs)"""
    u = _f32(v).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_from_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_rne(v):
    return bf16_from_bits(bf16_rne_bits(v))


def bf16_trunc(v):
    return (_f32(v).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split_bf16(v):
    """common.hpp split_bf16 (the weight packers): hi = bf16(x), lo = bf16(x - hi), both RNE"""
    v = _f32(v)
    hi = bf16_rne(v)
    return hi, bf16_rne(v - hi)


def split_bf16_staged(v):
    """conv1d_kernel.hpp write_one (activations, scheme 0): hi = x truncated to bf16, lo = bf16(x - hi) rounded"""
    v = _f32(v)
    hi = bf16_trunc(v)
    return hi, bf16_rne(v - hi)


def fp16_rne(v):
    """fp32 -> fp16 round-to-nearest-even (|v| >= 65520 -> inf), back as fp32"""
    with np.errstate(over="ignore"):
        return _f32(v).astype(np.float16).astype(np.float32)


def fp16_bits(v):
    with np.errstate(over="ignore"):
        return _f32(v).astype(np.float16).view(np.uint16)


def _minifloat_encode(v, ebits, mbits, bias, vmax):
    """codes of the sign / exponent / mantissa format with subnormals, RNE, saturating at +-vmax (inf included); the sign bit of the
    input is kept when the magnitude rounds to zero"""
    v = np.asarray(v, dtype=np.float64)
    a = np.minimum(np.abs(v), vmax)
    emin = 1 - bias
    _, ex = np.frexp(a)                                   # a = m * 2^ex, m in [0.5, 1)
    e = np.maximum(ex - 1, emin)
    n = np.rint(np.ldexp(a, -(e - mbits)))                # half-to-even; the scaling is exact
    r = np.minimum(np.ldexp(n, e - mbits), vmax)
    _, ex = np.frexp(r)
    e = np.maximum(ex - 1, emin)
    normal = r >= 2.0 ** emin
    mant = np.where(normal, np.ldexp(r, -(e - mbits)) - (1 << mbits), np.ldexp(r, -(emin - mbits))).astype(np.int64)
    expf = np.where(normal, e + bias, 0).astype(np.int64)
    sign = np.signbit(v).astype(np.int64)
    return ((sign << (ebits + mbits)) | (expf << mbits) | mant).astype(np.uint8)


def _minifloat_decode(code, ebits, mbits, bias):
    c = np.asarray(code).astype(np.int64)
    sign = np.where((c >> (ebits + mbits)) & 1, -1.0, 1.0)
    expf = (c >> mbits) & ((1 << ebits) - 1)
    mant = (c & ((1 << mbits) - 1)).astype(np.float64)
    val = np.where(expf == 0, np.ldexp(mant, 1 - bias - mbits), np.ldexp(mant + (1 << mbits), expf - bias - mbits))
    return sign * val


def e4m3_encode(v):
    """OCP e4m3 (bias 7, maximum 448, codes 0x7F / 0xFF are NaN and never produced): RNE, saturating"""
    return _minifloat_encode(v, 4, 3, 7, 448.0)


def e4m3_decode(code):
    return _minifloat_decode(code, 4, 3, 7)


def e2m3_encode(v):
    """OCP fp6 e2m3 (bias 1, 64 codes, maximum 7.5): RNE, saturating"""
    return _minifloat_encode(v, 2, 3, 1, 7.5)


def e2m3_decode(code):
    return _minifloat_decode(code, 2, 3, 1)


def e8m0_block_scale(mx):
    """conv_args.hpp e8m0_block_scale: biased exponent b of the smallest 2^(b - 127) with mx / 2^(b - 127) <= 7.5, from the fp32 product
    mx * (1 / 7.5f) by the integer formula (bits + 0x7FFFFF) >> 23, clamped to [13, 254]"""
    with np.errstate(over="ignore", under="ignore"):
        q = _f32(mx) * np.float32(np.float32(1.0) / np.float32(7.5))
    b = (q.view(np.uint32).astype(np.uint64) + 0x7FFFFF) >> 23
    return np.clip(b, E8M0_MIN, E8M0_MAX).astype(np.int64)


def _pow2(e):
    return np.ldexp(1.0, np.asarray(e, np.int64))


# ------------------------------------------------------------------------------------------------ operand splits
def _residual4k(v, h):
    """(v - fp16(v)) * 2^12 as the kernels form it in fp32 (exact for finite operands; -inf where fp16(v) overflowed)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return ((v - h) * np.float32(4096.0)).astype(np.float32)


def _blocks(a):
    assert a.shape[-1] % 16 == 0, "blocks are 16 consecutive channels"
    return a.reshape(*a.shape[:-1], a.shape[-1] // 16, 16)


def mx6_block(first, second):
    """One side of scheme 2: E8M0 byte per block and the e2m3 codes of both elements of each pair, (..., C) fp32 -> b (..., C/16),
    codes (..., C) x 2"""
    f, s = _blocks(_f32(first)), _blocks(_f32(second))
    with np.errstate(invalid="ignore"):
        mx = np.maximum(np.abs(f).max(-1), np.abs(s).max(-1))
    b = e8m0_block_scale(mx)
    inv = _pow2(127 - b)[..., None]
    with np.errstate(over="ignore", invalid="ignore"):
        cf = e2m3_encode(f.astype(np.float64) * inv).reshape(first.shape)
        cs = e2m3_encode(s.astype(np.float64) * inv).reshape(first.shape)
    return b, cf, cs


def split_weights(w, scheme):
    """Weight-side operands along the LAST axis (the contraction channels): a tuple of float64 arrays (see split_activations)"""
    w = _f32(w)
    if scheme == BF16X3:
        hi, lo = split_bf16(w)
        return hi.astype(np.float64), lo.astype(np.float64)
    h = fp16_rne(w)
    l4k = _residual4k(w, h)
    if scheme == F16_MX8:
        wf = e4m3_decode(e4m3_encode(np.clip(w, -448.0, 448.0)))
        wl = e4m3_decode(e4m3_encode(np.clip(l4k, -448.0, 448.0))) / 4096.0
        return h.astype(np.float64), wf, wl
    b, cw, cl = mx6_block(w, l4k)
    s = np.repeat(_pow2(b - 127), 16, axis=-1)
    return h.astype(np.float64), e2m3_decode(cw) * s, e2m3_decode(cl) * s / 4096.0


def split_activations(x, scheme):
    """Activation-side operands of the fp32 values the kernel stages (after its prologue and any 2^k scaling), blocks along the last
    axis.  Scheme 0: (hi, lo).  Schemes 1, 2: (fp16(x), estimate of x_l, estimate of x) -- the two correction operands with their
    scales applied, so that  y = xh wh + x_l~ W~ + x~ W_l~."""
    x = _f32(x)
    if scheme == BF16X3:
        hi, lo = split_bf16_staged(x)
        return hi.astype(np.float64), lo.astype(np.float64)
    h = fp16_rne(x)
    if scheme == F16_MX8:
        with np.errstate(invalid="ignore"):
            xl = np.clip((x - h).astype(np.float32), -0.109375, 0.109375)
        el = e4m3_decode(e4m3_encode(xl.astype(np.float64) * 4096.0)) / 4096.0
        ef = e4m3_decode(e4m3_encode(np.clip(x, -448.0, 448.0)))
        return h.astype(np.float64), el, ef
    b, cl, cf = mx6_block(_residual4k(x, h), x)
    s = np.repeat(_pow2(b - 127), 16, axis=-1)
    return h.astype(np.float64), e2m3_decode(cl) * s / 4096.0, e2m3_decode(cf) * s


def contract_split(xs, ws):
    """sum over the last axis of the scheme's products, operands from split_activations (N, C) / split_weights (M, C) -> (N, M)"""
    with np.errstate(invalid="ignore", over="ignore"):
        if len(xs) == 2:
            (xh, xl), (wh, wl) = xs, ws
            return xh @ wh.T + xh @ wl.T + xl @ wh.T
        (xh, xl, xf), (wh, wf, wl) = xs, ws
        return xh @ wh.T + xl @ wf.T + xf @ wl.T


def contract(x, w, scheme):
    """x (N, C) fp32 @ w (M, C)^T fp32 as scheme `scheme` computes it, float64 accumulation: xh wh + corrections"""
    return contract_split(split_activations(x, scheme), split_weights(w, scheme))


# ------------------------------------------------------------------------------------------------ convolutions
def conv1d_model(x, w, scheme):
    """Stride-1 "same" convolution of the STAGED activation x (B, T, C) fp32 (channels-last; zero padding is part of the staged image)
    with torch-layout weights w (C_out, C_in, K): (B, T, C_out) float64"""
    x, w = _f32(x), _f32(w)
    B, T, C = x.shape
    Co, Ci, K = w.shape
    assert Ci == C
    pad = K // 2
    xp = np.zeros((B, T + 2 * pad, C), np.float32)
    xp[:, pad:pad + T] = x
    xs = split_activations(xp, scheme)
    y = np.zeros((B, T, Co))
    for k in range(K):
        ws = split_weights(w[:, :, k], scheme)
        y += contract_split(tuple(a[:, k:k + T].reshape(B * T, C) for a in xs), ws).reshape(B, T, Co)
    return y


def conv1d_exact(x, w):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, T, C = x.shape
    K = w.shape[2]
    pad = K // 2
    xp = np.zeros((B, T + 2 * pad, C))
    xp[:, pad:pad + T] = x
    return sum(xp[:, k:k + T] @ w[:, :, k].T for k in range(K))


def dgrad_k(amax_bits):
    """exponent k of the data gradient's dy scaling 2^k (conv1d_kernel.hpp): biased exponent e of the amax word, k = 140 - e clamped
    to +-126, so that 2^13 <= max|dy| 2^k < 2^14"""
    e = (int(amax_bits) >> 23) & 0xFF
    return max(-126, min(126, 140 - e))


def transposed_weights(w):
    """A[ci][co][tap] = W[co][ci][K - 1 - tap]: the data gradient's operand as a (C_in, C_out, K) conv weight"""
    return np.ascontiguousarray(np.transpose(_f32(w), (1, 0, 2))[:, :, ::-1])


def dgrad_model(dy, w, scheme, amax_bits=None):
    """dx (B, T, C_in) float64 of a stride-1 "same" conv with weights w (C_out, C_in, K) for dy (B, T, C_out); scheme 2 stages
    dy * 2^k (k from the amax word) and multiplies the result by 2^-k"""
    dy = _f32(dy)
    k = 0
    if scheme == F16_MX6:
        k = dgrad_k(amax_bits)
        with np.errstate(over="ignore", under="ignore"):
            dy = dy * np.float32(2.0 ** k)
    return conv1d_model(dy, transposed_weights(w), scheme) * 2.0 ** -k


def dgrad_exact(dy, w):
    return conv1d_exact(dy, transposed_weights(w))


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad_taps(xhat, T_out, K, stride, upsample):
    """the K row-shifted views of the staged activation that meet dy[b, t]: xhat (B, T_in, C) -> list of (B, T_out, C);
    stride 1: source position t + k - K // 2 of the (nearest-x2 upsampled) image, stride 2 (K = 3): 2 t + k - 1; zeros outside"""
    assert stride in (1, 2) and not (stride == 2 and (upsample or K != 3))
    src = np.repeat(xhat, 2, axis=1) if upsample else xhat
    B, T_src, C = src.shape
    pad = K // 2 if stride == 1 else 1
    need = (T_out - 1) * stride + K
    xp = np.zeros((B, max(need, pad + T_src), C), src.dtype)
    xp[:, pad:pad + T_src] = src
    return [xp[:, k:k + (T_out - 1) * stride + 1:stride] for k in range(K)]


def wgrad_exact(dy, xhat, K, stride=1, upsample=False):
    """Weight gradient dw (C_out, C_in, K) float64 of a conv with output gradient dy (B, T_out, C_out) and STAGED activation xhat
    (B, T_in, C_in) (channels-last; after the launch's prologue: GroupNorm fold, SiLU, dropout), summed in float64"""
    dy, xhat = np.asarray(dy, np.float64), np.asarray(xhat, np.float64)
    B, T_out, Co = dy.shape
    a = dy.reshape(B * T_out, Co)
    taps = _wgrad_taps(xhat, T_out, K, stride, upsample)
    return np.stack([a.T @ x.reshape(B * T_out, -1) for x in taps], axis=-1)


WGRAD_PRODUCTS = ("lo_hi", "hi_lo", "hi_hi")    # (dy part, xhat part) of mfma_x3's three products, in its order


def wgrad_products(dy, xhat, K, stride=1, upsample=False):
    """The three products of mfma_x3 in wgrad_kernel, each (C_out, C_in, K) float64 with exact products and float64 sums, keyed by
    WGRAD_PRODUCTS: both operands are split with split_bf16 (RNE / RNE, common.hpp) into hi + lo; "lo_hi" = dy_lo xhat_hi, "hi_lo" =
    dy_hi xhat_lo, "hi_hi" = dy_hi xhat_hi (lo lo is not formed)."""
    dy, xhat = _f32(dy), _f32(xhat)
    B, T_out, Co = dy.shape
    dh, dl = (p.astype(np.float64).reshape(B * T_out, Co) for p in split_bf16(dy))
    xh, xl = split_bf16(xhat)
    th = [x.reshape(B * T_out, -1) for x in _wgrad_taps(xh.astype(np.float64), T_out, K, stride, upsample)]
    tl = [x.reshape(B * T_out, -1) for x in _wgrad_taps(xl.astype(np.float64), T_out, K, stride, upsample)]
    return {"lo_hi": np.stack([dl.T @ t for t in th], axis=-1), "hi_lo": np.stack([dh.T @ t for t in tl], axis=-1),
            "hi_hi": np.stack([dh.T @ t for t in th], axis=-1)}


def wgrad_model(dy, xhat, K, stride=1, upsample=False, leave_out=None, products=None):
    """wgrad_exact as wgrad_kernel forms it: the sum of wgrad_products.  ``leave_out``: one of the cross products ("lo_hi" / "hi_lo")
    is dropped -- only for sizing a test's bar against the error such a defect would make.  ``products``: a wgrad_products result of
    the same operands, to form several variants without repeating the contractions."""
    assert leave_out in (None, "lo_hi", "hi_lo")
    p = products if products is not None else wgrad_products(dy, xhat, K, stride, upsample)
    return sum(p[n] for n in WGRAD_PRODUCTS if n != leave_out)


def wgrad_channel_err(dw, ref):
    """channel_err of a weight gradient (C_out, C_in, K): per OUTPUT channel (the first axis), the worst one"""
    return channel_err(np.moveaxis(np.asarray(dw, np.float64), 0, -1), np.moveaxis(np.asarray(ref, np.float64), 0, -1))


def staged_dropout(xhat, seed, site, p):
    """the dropout stage of a prologue on the staged activation xhat (B, T, C) fp32: kept values times 1 / (1 - p) in fp32, element
    index t * C + c (oracle/dropout.py)"""
    from .dropout import dropout_scale_mask
    xhat = _f32(xhat)
    B, T, C = xhat.shape
    return (xhat * dropout_scale_mask(seed, site, B, T, C, p)).astype(np.float32)


def staged_gn(x, a, s):
    """a x + s in fp32 as a GroupNorm-only prologue stages it (one fused multiply-add).  x (B, T, C), a / s (B, C)"""
    return (np.asarray(x, np.float64) * np.asarray(a, np.float64)[:, None, :] + np.asarray(s, np.float64)[:, None, :]).astype(np.float32)


def staged_gn_silu(x, a, s):
    """silu(a x + s) in fp32 as a GN + SiLU launch stages it: one fused multiply-add, then u / (1 + exp(-u)).  x (B, T, C), a / s (B, C)"""
    u = (np.asarray(x, np.float64) * np.asarray(a, np.float64)[:, None, :] + np.asarray(s, np.float64)[:, None, :]).astype(np.float32)
    with np.errstate(over="ignore"):
        return (u / (np.float32(1.0) + np.exp(-u))).astype(np.float32)


def channel_err(y, ref):
    """e_m of the kernel tests: max|y - ref| / max|ref| per output channel (last axis), the worst channel"""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    d = np.abs(y - ref).reshape(-1, ref.shape[-1]).max(0)
    m = np.abs(ref).reshape(-1, ref.shape[-1]).max(0)
    return float((d / np.maximum(m, 1e-300)).max())


# ------------------------------------------------------------------------------------------------ packed-weight layouts
# Per lane fragments of 16 bytes, lane l = 16 kq + r: row = 16 cob + r of the operand matrix A[row][k] (modes 0, 2, 3: row = co,
# k = ci, A = W[co][ci][tap]; modes 1, 5: row = ci, k = co, A = W[co][ci][K - 1 - tap]).
#   modes 0, 1 (bf16x3): packed[chunk][tap][cob][hl][lane][8 x bf16], k = 32 chunk + 8 kq + j; hl 0 = hi, 1 = lo
#   modes 2, 3, 5:       packed[chunk][tap][cob][f][lane][16 bytes], 64-channel chunks; f 0 / 1: fp16(A) of k = 64 chunk + 8 kq + j and
#                        64 chunk + 32 + 8 kq + j; mode 2: f 2 / 3 = e4m3(A) / e4m3(A_l 2^12) of k = 64 chunk + 16 kq + j (one byte each);
#                        modes 3, 5: the 32 e2m3 codes of the lane's block (element 2i = A, 2i + 1 = A_l 2^12 of k = 64 chunk + 16 kq + i,
#                        divided by the block's 2^e) as one little-endian stream of 192 bits = f 2 bytes 0..15 + f 3 bytes 0..7, the
#                        E8M0 byte in f 3 byte 8 (dword 2), bytes 9..15 zero
def tile_co(rows):
    return 128 if rows % 128 == 0 else (64 if rows % 64 == 0 else 32)


def pack_geometry(C_out, C_in, K, mode):
    tr = mode in (1, 5)
    rows, kdim = (C_in, C_out) if tr else (C_out, C_in)
    tile = tile_co(rows)
    ncob_pad = (rows + tile - 1) // tile * tile // 16
    ch = 32 if mode in (0, 1) else 64
    nchunks = (kdim + ch - 1) // ch
    return dict(rows=rows, kdim=kdim, ncob_pad=ncob_pad, ch=ch, nchunks=nchunks, transposed=tr,
                nbytes=nchunks * K * ncob_pad * (2 if ch == 32 else 4) * 64 * 16)


def operand_matrix(w, mode, geometry=None):
    """A[row][k][tap] fp32, zero-padded to (16 ncob_pad, nchunks * ch, K)"""
    w = _f32(w)
    g = geometry or pack_geometry(w.shape[0], w.shape[1], w.shape[2], mode)
    a = np.transpose(w, (1, 0, 2))[:, :, ::-1] if g["transposed"] else w
    out = np.zeros((g["ncob_pad"] * 16, g["nchunks"] * g["ch"], w.shape[2]), np.float32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def decode_packed(buf, C_out, C_in, K, mode):
    """Packed bytes -> dict of arrays indexed [row][k][tap] (E8M0: [row][k / 16][tap]):
    modes 0, 1: hi, lo (uint16 bf16 bits); mode 2: h (uint16 fp16 bits), c0, c1 (uint8 e4m3 codes of A, A_l 2^12);
    modes 3, 5: h, c0, c1 (e2m3 codes), e8m0 (uint8), tail (the 7 bytes after the E8M0 byte, all zero in a valid buffer)"""
    g = pack_geometry(C_out, C_in, K, mode)
    buf = np.ascontiguousarray(np.asarray(buf, np.uint8)).reshape(-1)
    assert buf.size == g["nbytes"], (buf.size, g["nbytes"])
    nc, P = g["nchunks"], g["ncob_pad"]
    R = P * 16
    if mode in (0, 1):
        v = buf.view(np.uint16).reshape(nc, K, P, 2, 4, 16, 8)               # chunk, tap, cob, hl, kq, r, j
        v = v.transpose(3, 2, 5, 0, 4, 6, 1).reshape(2, R, nc * 32, K)       # hl, (cob, r), (chunk, kq, j), tap
        return dict(hi=v[0], lo=v[1])
    v = buf.reshape(nc, K, P, 4, 4, 16, 16)                                   # chunk, tap, cob, f, kq, r, byte
    h = np.ascontiguousarray(v[:, :, :, 0:2]).view(np.uint16)                 # chunk, tap, cob, half, kq, r, j (8)
    h = h.transpose(2, 5, 0, 3, 4, 6, 1).reshape(R, nc * 64, K)              # (cob, r), (chunk, half, kq, j), tap
    if mode == 2:
        c = v[:, :, :, 2:4].transpose(3, 2, 5, 0, 4, 6, 1).reshape(2, R, nc * 64, K)   # f, (cob, r), (chunk, kq, byte), tap
        return dict(h=h, c0=c[0], c1=c[1])
    stream = np.concatenate([v[:, :, :, 2], v[:, :, :, 3, :, :, 0:8]], axis=-1)        # chunk, tap, cob, kq, r, 24 bytes
    bits = np.unpackbits(stream, axis=-1, bitorder="little").reshape(nc, K, P, 4, 16, 32, 6)
    codes = (bits.astype(np.uint8) << np.arange(6, dtype=np.uint8)).sum(-1).astype(np.uint8)   # ..., 32 codes: 2 i = A, 2 i + 1 = A_l
    codes = codes.reshape(nc, K, P, 4, 16, 16, 2).transpose(6, 2, 4, 0, 3, 5, 1).reshape(2, R, nc * 64, K)
    e8 = v[:, :, :, 3, :, :, 8].transpose(2, 4, 0, 3, 1).reshape(R, nc * 4, K)         # (cob, r), (chunk, kq), tap
    tail = v[:, :, :, 3, :, :, 9:16]
    return dict(h=h, c0=codes[0], c1=codes[1], e8m0=e8, tail=tail)


def pack_model(w, mode):
    """What tq_pack_conv_weight must produce for w (C_out, C_in, K), in the arrays of decode_packed"""
    a = operand_matrix(w, mode)                    # row, k, tap
    at = np.ascontiguousarray(a.transpose(0, 2, 1))   # row, tap, k: blocks along the last axis
    back = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1))
    if mode in (0, 1):
        hi = bf16_rne(a)
        return dict(hi=bf16_rne_bits(a), lo=bf16_rne_bits(a - hi))
    h = fp16_rne(at)
    l4k = _residual4k(at, h)
    if mode == 2:
        return dict(h=back(fp16_bits(at)), c0=back(e4m3_encode(np.clip(at, -448.0, 448.0))),
                    c1=back(e4m3_encode(np.clip(l4k, -448.0, 448.0))))
    b, c0, c1 = mx6_block(at, l4k)
    return dict(h=back(fp16_bits(at)), c0=back(c0), c1=back(c1), e8m0=back(b.astype(np.uint8)),
                tail=np.zeros(1, np.uint8))


# ------------------------------------------------------------------------------------------------ range table
def range_table(scheme, w_scales=(1.0, 1e-3, 1e-5, 1e-6, 1e-7, 1e-9), x_scales=(1e3, 1.0, 1e-3, 1e-5, 1e-7), C=64, K=5, M=32, N=256, seed=0):
    """model-versus-exact error (max|y - exact| / max|exact|) of y = x w over C K contraction entries, weights ~ w_scale / sqrt(C K),
    activations ~ x_scale: rows of (w_scale, x_scale, error)"""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((N, C * K)).astype(np.float32)
    w0 = (rng.standard_normal((M, C * K)) / np.sqrt(C * K)).astype(np.float32)
    rows = []
    for ws in w_scales:
        for xs in x_scales:
            x, w = (x0 * np.float32(xs)).astype(np.float32), (w0 * np.float32(ws)).astype(np.float32)
            ex = x.astype(np.float64) @ w.astype(np.float64).T
            rows.append((ws, xs, float(np.abs(contract(x, w, scheme) - ex).max() / np.abs(ex).max())))
    return rows
