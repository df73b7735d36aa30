"""Host mirror of the HIP path's dropout masks.  TEST INFRASTRUCTURE ONLY.

The kernels draw no random numbers: an element is kept iff `drop_hash(seed, row, col) >= thr` (acai_omr_amd/csrc/common.h), each
kernel regenerating the hash from its own coordinates.  This module restates that arithmetic on torch int64 tensors (every product
masked back to 32 bits), so that a test can rebuild the exact keep mask of any call and run a float64 reference under it.

The probability reaches the kernels as a C float: thr = (uint32_t)((double)p_f32 * 2^32) and scale = 1.0f / (1.0f - p_f32) in fp32.
Both are formed here from the fp32 value of p - the double p gives another threshold (p = 0.1: 429496729 instead of 429496736).

Coordinates:
  - acai_dropout_add: row and column of the 2-D tensor (train.hip, dropout_add_kernel);
  - attention probabilities: row = h * total_q + cu_q[b] + q (the query's packed row, offset by head), col = the key's index inside
    its own sequence (attn_varlen.hip / attn_bwd.hip).
"""
import numpy as np
import torch

M32 = 0xFFFFFFFF


def _u32(x):
    return torch.as_tensor(x, dtype=torch.int64) & M32


def _mul32(x, c):
    """(x * c) mod 2^32 for x in [0, 2^32): by 16-bit halves, so that no int64 product overflows."""
    return ((x & 0xFFFF) * c + ((((x >> 16) * c) & 0xFFFF) << 16)) & M32


def drop_hash(seed, row, col):
    """common.h drop_hash on broadcastable int tensors (or ints): the 32-bit hash as an int64 tensor in [0, 2^32)."""
    row, col = _u32(row), _u32(col)
    x = _mul32(row, 0x9E3779B1) ^ _mul32(col, 0x85EBCA77) ^ (int(seed) & M32)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x2C1B3C6D)
    x = x ^ (x >> 12)
    x = _mul32(x, 0x297A2D39)
    return x ^ (x >> 15)


def p_f32(p):
    return float(np.float32(p))


def drop_threshold(p):
    """The kernels' 32-bit keep threshold for dropout probability p (taken as the C float the ABI receives)."""
    return int(p_f32(p) * 4294967296.0)


def drop_scale(p):
    """1.0f / (1.0f - p) in fp32, as the entry points form it."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _index(n):
    return torch.arange(int(n), dtype=torch.int64) if isinstance(n, (int, np.integer)) else torch.as_tensor(n, dtype=torch.int64)


def dropout_keep(seed, rows, cols, p):
    """Keep mask (bool [len(rows), len(cols)]) of acai_dropout_add.  rows / cols: a count (indices 0..n-1) or a 1-D tensor of the
    tensor's row / column indices (a test maps another packing's rows onto the kernel's this way)."""
    r, c = _index(rows), _index(cols)
    return drop_hash(seed, r.unsqueeze(1), c.unsqueeze(0)) >= drop_threshold(p)


def attn_keep(seed, p, h, total_q, q_row0, lq, lk):
    """Keep mask (bool [lq, lk]) of head h of the sequence whose queries start at packed row q_row0 of a batch of total_q query rows."""
    rows = int(h) * int(total_q) + int(q_row0) + torch.arange(int(lq), dtype=torch.int64)
    return drop_hash(seed, rows.unsqueeze(1), torch.arange(int(lk), dtype=torch.int64).unsqueeze(0)) >= drop_threshold(p)


def multiplier(keep, p, dtype=torch.float64):
    """keep * scale: what a kept element is multiplied by (0 where dropped)."""
    return keep.to(dtype) * drop_scale(p)
