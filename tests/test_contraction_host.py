"""The CPU bit-model of the conv contraction schemes (oracle/contraction.py) checked on its own, without a GPU: the rounders against
exhaustive enumeration of their code sets and against torch / numpy conversions, the E8M0 block scale at its edges, the packed-weight
decoder against a hand-built buffer, and the model's own error against exact arithmetic.  `pytest -s` prints the range table of
DESIGN.md section 3."""

import numpy as np
import pytest
import torch

from oracle import contraction as M


def _nearest_even(values, codes, v):
    """brute force RNE onto a sorted table of non-negative values: the nearest entry, ties to the even code, saturating"""
    out = np.empty(v.shape, np.int64)
    for i, a in enumerate(np.abs(v)):
        d = np.abs(values - min(a, values[-1]))
        best = np.flatnonzero(d == d.min())
        pick = best[0] if len(best) == 1 else [b for b in best if codes[b] % 2 == 0][0]
        out[i] = codes[pick]
    return out


@pytest.mark.parametrize("name,ncodes,signbit,vmax", [("e2m3", 64, 0x20, 7.5), ("e4m3", 256, 0x80, 448.0)])
def test_minifloat_rounders_exhaustively(name, ncodes, signbit, vmax):
    enc, dec = getattr(M, name + "_encode"), getattr(M, name + "_decode")
    codes = np.array([c for c in range(ncodes) if not (name == "e4m3" and (c & 0x7F) == 0x7F)])   # (e4m3: 0x7F / 0xFF are NaN)
    vals = dec(codes)
    pos = codes[codes < signbit]
    pv = vals[codes < signbit]
    assert len(codes) == (64 if name == "e2m3" else 254)
    assert np.all(np.diff(pv) > 0) and pv[0] == 0 and pv[-1] == vmax                    # monotone code order, documented maximum
    assert np.array_equal(vals[codes >= signbit], -pv)
    assert np.array_equal(enc(vals), codes)                                              # every code is a fixed point (-0 included)
    if name == "e2m3":   # the 32 magnitudes of OCP fp6 e2m3: eighths below 1, then 1/8, 1/4, 1/2 steps
        assert np.array_equal(pv, np.concatenate([np.arange(8) / 8, 1 + np.arange(8) / 8, 2 + np.arange(8) / 4, 4 + np.arange(8) / 2]))
    else:
        assert dec(np.array([0x01, 0x08, 0x38, 0x7E])).tolist() == [2.0 ** -9, 2.0 ** -6, 1.0, 448.0]
    # every midpoint between neighbours (the ties), one step to either side of it, and beyond the maximum
    mid = (pv[1:] + pv[:-1]) / 2
    probe = np.concatenate([mid, np.nextafter(mid, 0), np.nextafter(mid, np.inf), [vmax * 1.01, vmax * 4, 1e30, np.inf, pv[1] / 4]])
    want = _nearest_even(pv, pos, probe)
    assert np.array_equal(enc(probe), want)
    assert np.array_equal(enc(-probe), want | signbit)
    rng = np.random.default_rng(0)
    dense = np.concatenate([rng.uniform(0, vmax * 1.1, 4000), np.exp(rng.uniform(np.log(pv[1] / 8), np.log(vmax), 4000))])
    assert np.array_equal(enc(dense), _nearest_even(pv, pos, dense))


def test_bf16_and_fp16_rounders_against_torch_and_numpy():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.standard_normal(20000) * np.exp(rng.uniform(-40, 40, 20000)),
                        [0.0, 1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -9, 65504.0, 65519.9, 65520.0, 2.0 ** -24, 2.0 ** -25, 6e-8]]).astype(np.float32)
    t = torch.from_numpy(v)
    assert np.array_equal(M.bf16_rne(v), t.to(torch.bfloat16).float().numpy())
    assert np.array_equal(M.bf16_rne_bits(v), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    with np.errstate(over="ignore"):
        assert np.array_equal(M.fp16_rne(v), v.astype(np.float16).astype(np.float32))
    assert np.array_equal(M.fp16_rne(v), t.to(torch.float16).float().numpy())
    hi, lo = M.split_bf16(v)
    assert np.array_equal(hi, M.bf16_rne(v)) and np.array_equal(lo, M.bf16_rne(v - hi))
    th, tl = M.split_bf16_staged(v)
    assert np.all(np.abs(th) <= np.abs(v)) and np.array_equal(th.view(np.uint32) & 0xFFFF, np.zeros(v.shape, np.uint32))
    fin = np.abs(v) < 1e30
    # both splits reproduce x to 2^-16 (hi truncated: the remainder has up to 2^-7 |x| and 8 bits of it are kept; hi rounded: 2^-17)
    assert np.all(np.abs(th.astype(np.float64) + tl - v)[fin] <= np.abs(v[fin]) * 2.0 ** -16)
    assert np.all(np.abs(hi.astype(np.float64) + lo - v)[fin] <= np.abs(v[fin]) * 2.0 ** -17)


def test_e8m0_block_scale_edges():
    f = lambda x: int(M.e8m0_block_scale(np.float32(x)).reshape(-1)[0])
    for e in (-100, -20, -3, 0, 1, 7, 40, 100):
        assert f(2.0 ** e) == 127 + e - 2                              # 2^e / 2^(e - 2) = 4 <= 7.5 < 8
        top = np.float32(7.5 * 2.0 ** e)
        assert f(top) == 127 + e                                        # 7.5 * 2^e itself still fits 2^e ...
        assert f(np.nextafter(top, np.float32(0))) == 127 + e
        assert f(np.nextafter(top, np.float32(np.inf))) == 127 + e + 1  # ... one ulp more does not
    assert f(0.0) == 13 and f(1e-45) == 13 and f(7.5 * 2.0 ** -114) == 13 and f(7.6 * 2.0 ** -114) == 14   # lower clamp
    assert f(3.0e38) == 252 and f(np.inf) == 254                                                           # upper clamp
    # never saturating inside the clamps: max / 2^e <= 7.5, and 2^e is the smallest such power of two
    rng = np.random.default_rng(2)
    mx = np.exp(rng.uniform(-70, 80, 5000)).astype(np.float32)
    b = M.e8m0_block_scale(mx)
    assert np.all(mx.astype(np.float64) * 2.0 ** (127 - b) <= 7.5) and np.all(mx.astype(np.float64) * 2.0 ** (128 - b) > 7.5)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 5])
def test_packed_layout_decoder_against_a_hand_built_buffer(mode):
    """decode_packed reads the layout documented in conv1d_mfma.hip: the buffer is built here lane by lane from those comments (a loop
    over fragments, nothing shared with the vectorised decoder)."""
    rng = np.random.default_rng(mode)
    C_out, C_in, K = (32, 96, 3) if mode in (0, 2, 3) else (96, 32, 3)
    w = (rng.standard_normal((C_out, C_in, K)) * np.exp(rng.uniform(-6, 3, (C_out, C_in, K)))).astype(np.float32)
    g = M.pack_geometry(C_out, C_in, K, mode)
    assert (g["rows"], g["kdim"], g["ncob_pad"]) == (32, 96, 2)
    A = M.operand_matrix(w, mode)
    want = M.pack_model(w, mode)
    nfrag = 2 if mode < 2 else 4
    buf = np.zeros((g["nchunks"], K, g["ncob_pad"], nfrag, 64, 16), np.uint8)
    for chunk in range(g["nchunks"]):
        for tap in range(K):
            for cob in range(g["ncob_pad"]):
                for lane in range(64):
                    row, kq = cob * 16 + (lane & 15), lane >> 4
                    if mode < 2:
                        a = A[row, chunk * 32 + 8 * kq:chunk * 32 + 8 * kq + 8, tap]
                        hi = M.bf16_rne(a)
                        buf[chunk, tap, cob, 0, lane] = M.bf16_rne_bits(a).view(np.uint8)
                        buf[chunk, tap, cob, 1, lane] = M.bf16_rne_bits(a - hi).view(np.uint8)
                        continue
                    for half in range(2):
                        k0 = chunk * 64 + 32 * half + 8 * kq
                        buf[chunk, tap, cob, half, lane] = M.fp16_bits(A[row, k0:k0 + 8, tap]).view(np.uint8)
                    blk = A[row, chunk * 64 + 16 * kq:chunk * 64 + 16 * kq + 16, tap]
                    l4k = (blk - M.fp16_rne(blk)) * np.float32(4096)
                    if mode == 2:
                        buf[chunk, tap, cob, 2, lane] = M.e4m3_encode(np.clip(blk, -448, 448))
                        buf[chunk, tap, cob, 3, lane] = M.e4m3_encode(np.clip(l4k, -448, 448))
                        continue
                    b = int(M.e8m0_block_scale(np.float32(max(np.abs(blk).max(), np.abs(l4k).max()))).reshape(-1)[0])
                    word = 0
                    for i in range(16):
                        word |= int(M.e2m3_encode(float(blk[i]) * 2.0 ** (127 - b))) << (12 * i)
                        word |= int(M.e2m3_encode(float(l4k[i]) * 2.0 ** (127 - b))) << (12 * i + 6)
                    stream = np.frombuffer(word.to_bytes(24, "little"), np.uint8)
                    buf[chunk, tap, cob, 2, lane] = stream[:16]
                    buf[chunk, tap, cob, 3, lane, :8] = stream[16:]
                    buf[chunk, tap, cob, 3, lane, 8] = b
    got = M.decode_packed(buf.reshape(-1), C_out, C_in, K, mode)
    for key in want:
        if key == "tail":
            assert not got["tail"].any()
        else:
            assert np.array_equal(got[key], want[key]), key
    if mode in (3, 5):   # the 32 pad columns of the second chunk are all-zero blocks: lowest scale, zero codes
        assert np.all(got["e8m0"][:, 6:8] == 13) and not got["c0"][:, 96:].any() and not got["h"][:, 96:].any()


O1_BOUND = {M.BF16X3: 2.0 ** -15, M.F16_MX8: 2.0 ** -14, M.F16_MX6: 2.0 ** -14}


@pytest.mark.parametrize("scheme", M.SCHEMES)
def test_model_error_on_order_one_data(scheme):
    """What each scheme drops, per product and relative to it: bf16x3 the xl wl term (<= 2^-8 2^-8 with a truncated hi) and the rounding
    of the lo parts (2^-17 each): < 2^-15; the fp16 schemes round two corrections of <= 2^-11 each to 4 (e4m3) or, relative to the block
    maximum, 3.9 (e2m3) bits: <= 2^-14.  Over 320 random-sign products the sum's error relative to the largest output stays below the
    per-product bound; it is also not zero -- the model is not exact arithmetic."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 64, 64)).astype(np.float32)
    w = (rng.standard_normal((32, 64, 5)) / np.sqrt(320)).astype(np.float32)
    ex = M.conv1d_exact(x, w)
    err = np.abs(M.conv1d_model(x, w, scheme) - ex).max() / np.abs(ex).max()
    print(f"{M.SCHEME_NAME[scheme]}: model against exact on O(1) data {err:.2e}")
    assert 1e-6 < err < O1_BOUND[scheme]
    # one contraction = the conv's centre tap
    y1 = M.contract(x.reshape(-1, 64), w[:, :, 2], scheme)
    e1 = np.abs(y1 - x.reshape(-1, 64).astype(np.float64) @ w[:, :, 2].astype(np.float64).T).max() / np.abs(y1).max()
    assert 1e-7 < e1 < O1_BOUND[scheme]


def test_data_gradient_scaling_exponent():
    bits = lambda v: int(np.float32(v).view(np.uint32))
    for v in (1e-9, 3e-5, 1.0, 2e3, 8191.9, 8192.0, 16383.0):
        k = M.dgrad_k(bits(v))
        assert 2.0 ** 13 <= v * 2.0 ** k < 2.0 ** 14
    assert M.dgrad_k(0) == 126 and M.dgrad_k(bits(1e-45)) == 126 and M.dgrad_k(bits(np.inf)) == -115 and M.dgrad_k(bits(3e38)) == -114
    assert M.dgrad_k(bits(1.0) + (3 << 23)) == M.dgrad_k(bits(1.0)) - 3      # an amax word 8 times too large: three binades less
    # the scaling is exact and undone exactly: scheme 2 on dy 2^-30 equals scheme 2 on dy, times 2^-30
    rng = np.random.default_rng(4)
    dy = rng.standard_normal((1, 40, 64)).astype(np.float32)
    w = (rng.standard_normal((64, 64, 3)) / 14).astype(np.float32)
    a = M.dgrad_model(dy, w, M.F16_MX6, bits(np.abs(dy).max()))
    b = M.dgrad_model(dy * np.float32(2.0 ** -30), w, M.F16_MX6, bits(np.abs(dy).max() * 2.0 ** -30))
    assert np.array_equal(a * 2.0 ** -30, b)
    ex = M.dgrad_exact(dy, w)
    assert np.abs(a - ex).max() / np.abs(ex).max() < 2.0 ** -14


def test_range_table(capsys):
    """The envelope of each scheme by the model (printed for DESIGN.md): bf16x3 is flat over the whole sweep; the fp16 schemes keep their
    O(1) error only while both operands stay in fp16's normal range."""
    rows = {s: M.range_table(s, N=64, M=16) for s in M.SCHEMES}
    with capsys.disabled():
        print("\nmodel against exact fp64, max|y - exact| / max|exact| (C_in K = 320; weights ~ scale / sqrt(320), activations ~ scale)")
        print("weights  activations   " + "  ".join(f"{M.SCHEME_NAME[s]:>9s}" for s in M.SCHEMES))
        for i, (ws, xs, _) in enumerate(rows[M.BF16X3]):
            print(f"{ws:7.0e}  {xs:11.0e}   " + "  ".join(f"{rows[s][i][2]:9.1e}" for s in M.SCHEMES))
    cell = lambda s, ws, xs: next(e for a, b, e in rows[s] if a == ws and b == xs)
    assert max(e for _, _, e in rows[M.BF16X3]) < 2.0 ** -15
    for s in (M.F16_MX8, M.F16_MX6):
        assert cell(s, 1.0, 1.0) < 2.0 ** -14
    assert cell(M.F16_MX6, 1.0, 1e3) < 2.0 ** -14 and cell(M.F16_MX6, 1e-3, 1e-3) < 2.0 ** -14
    # outside the envelope the default scheme is at the per-cent level: weights of rms 5.6e-9 ... 5.6e-8 (1e-7, 1e-9 over sqrt(320))
    assert cell(M.F16_MX6, 1e-7, 1.0) > 1e-2 and cell(M.F16_MX6, 1e-9, 1.0) > 1e-2 and cell(M.F16_MX6, 1.0, 1e-7) > 1e-3
