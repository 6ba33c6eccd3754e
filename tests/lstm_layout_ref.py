"""The memory layouts of the LSTM kernels, stated once in Python (numpy only; include/mt_hip.h and csrc/lstm.hip hold the originals).

  hx      f16  hx[b/32][t][dir][k/16][((k/8)%2)*32 + b%32][k%8]     every step's h as the MFMA operand image (mt_lstm_hx_bytes)
  cx, dh  f32  [b/32][t][dir][k/8][k%8][b%32]                       cell states / gradient of h (mt_lstm_cx_bytes)
  rows         m = t B + b, columns col_off + dir Hv + j            what the re-layout kernels write for the GEMMs

tests/test_post_optim_ref_cpu.py checks the encoders index by index against these formulas; tests/test_gpu_lstm_layouts.py builds every input
of the pure permutation kernels with them."""
import numpy as np


def groups(B):
    return (B + 31) // 32


def hx_index(b, t, d, k, T, H):
    """element offset (in f16 words) of h[b][t][d][k] in the hx image"""
    return (((((b // 32) * T + t) * 2 + d) * (H // 16) + k // 16) * 64 + ((k // 8) % 2) * 32 + b % 32) * 8 + k % 8


def cell_index(b, t, d, k, T, H):
    """element offset (in floats) of a[b][t][d][k] in the cx / dh image"""
    return (((((b // 32) * T + t) * 2 + d) * (H // 8) + k // 8) * 8 + k % 8) * 32 + b % 32


def hx_words(B, T, H):
    return groups(B) * T * 2 * (H // 16) * 64 * 8


def cell_words(B, T, H):
    return groups(B) * T * 2 * (H // 8) * 8 * 32


def _grid(B, T, H):
    return np.meshgrid(np.arange(B), np.arange(T), np.arange(2), np.arange(H), indexing="ij")


def encode_hx(h, pad_bits):
    """h [B][T][2][H] as f16 (or its uint16 bits) -> flat uint16 image; batch slots >= B hold pad_bits"""
    h = np.asarray(h)
    bits = h.view(np.uint16) if h.dtype == np.float16 else h.astype(np.uint16)
    B, T, _, H = bits.shape
    assert H % 16 == 0 and bits.shape[2] == 2
    img = np.full(hx_words(B, T, H), pad_bits, dtype=np.uint16)
    b, t, d, k = _grid(B, T, H)
    img[hx_index(b, t, d, k, T, H)] = bits
    return img


def decode_hx(image, B, T, H):
    """flat uint16 image -> uint16 bits [B][T][2][H]"""
    b, t, d, k = _grid(B, T, H)
    return np.asarray(image).reshape(-1)[hx_index(b, t, d, k, T, H)]


def encode_cell(a, pad):
    """a [B][T][2][H] f32 -> flat float32 image; batch slots >= B hold pad"""
    a = np.asarray(a, dtype=np.float32)
    B, T, _, H = a.shape
    assert H % 8 == 0 and a.shape[2] == 2
    img = np.full(cell_words(B, T, H), pad, dtype=np.float32)
    b, t, d, k = _grid(B, T, H)
    img[cell_index(b, t, d, k, T, H)] = a
    return img


def decode_cell(image, B, T, H):
    b, t, d, k = _grid(B, T, H)
    return np.asarray(image).reshape(-1)[cell_index(b, t, d, k, T, H)]


def rows_from_h(h, Hv, col_off, ld, fill):
    """h [B][T][2][H] -> rows [T B][ld] with row m = t B + b, column col_off + dir Hv + j for j < Hv; `fill` everywhere else"""
    B, T, _, H = h.shape
    out = np.full((T * B, ld), fill, dtype=h.dtype)
    for d in range(2):
        out[:, col_off + d * Hv:col_off + (d + 1) * Hv] = h[:, :, d, :Hv].transpose(1, 0, 2).reshape(T * B, Hv)
    return out


def distinct_f16_bits(shape, seed):
    """random finite f16 bit patterns, all distinct while there are enough of them (63 488), else a second shuffled round"""
    rng = np.random.default_rng(seed)
    allb = np.arange(65536, dtype=np.uint32)
    finite = allb[((allb >> 10) & 31) != 31].astype(np.uint16)
    n = int(np.prod(shape))
    parts, left = [], n
    while left > 0:
        parts.append(rng.permutation(finite)[:left])
        left -= parts[-1].size
    return np.concatenate(parts).reshape(shape)


def bf16_bits_rne_f32(x):
    """float32 values -> their bf16 bits, rounded to nearest even (plain integer arithmetic on the float32 bits; finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_rne(f16_bits):
    """uint16 f16 bits -> the bf16 bits of the value rounded to nearest even"""
    return bf16_bits_rne_f32(np.asarray(f16_bits, dtype=np.uint16).view(np.float16).astype(np.float32))
