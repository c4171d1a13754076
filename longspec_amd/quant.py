"""Weight quantisation on the host -- pure torch, runs on CPU: row-wise FP8 (OCP e4m3fn) and block-wise OCP MX FP4.

FP8
---

The definition, shared bit for bit with the device quantiser ``ls_linear_w8_quantize`` (csrc/gemm_w8.hip):

    amax    = max_k |float(W[n, k])|
    s[n]    = 2^ceil(log2(amax / 448))      (``pow2=True``; exponent arithmetic, exponent >= -120;  amax == 0 -> 1)
    s[n]    = amax / 448                    (``pow2=False``: checkpoints quantised elsewhere)
    q[n, k] = e4m3fn(float(W[n, k]) / s[n]) round to nearest even, saturating at +-448, never the NaN encoding

so that ``224 s < amax <= 448 s``.  With a power-of-two scale ``q * s`` is exactly representable in fp16 and bf16, which is
what makes the 8-bit decode path bit-identical to the 16-bit one on the de-quantised weights ("8-bit weights").

De-quantising and quantising again returns the same VALUES.  It returns the same ``(q, s)`` pair too, except for a row whose
``amax / s`` lies in (224, 232]: its largest byte rounds down to 224, the de-quantised row has ``amax' = 224 s``, and the
definition above then gives ``(2 q, s / 2)`` -- the same numbers, one exponent moved from the scale into the bytes.

MXFP4
-----
The definition, shared bit for bit with the device quantiser ``ls_linear_w4_quantize`` (csrc/gemm_w4.hip):

    element   e2m1: a sign bit and the magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6} (codes 0..7); two per byte, the lower k in the
              low nibble
    block     32 consecutive k of one row share one e8m0 byte b, scale 2^(b - 127)
    amax      = max |float(W[n, k])| over the block
    E         = ceil(log2(amax / 6)) by exponent arithmetic (amax = m 2^ex, m in [0.5, 1), 6 = 0.75 * 2^3:
                E = ex - 3 + (m > 0.75)), clamped to [-13, 13];  amax == 0 -> E = 0;  b = E + 127
    q[n, k]   = e2m1(float(W[n, k]) / 2^E), round to nearest, ties to the even mantissa bit (0.25 -> 0, 0.75 -> 1, 1.25 -> 1,
                1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), saturating at +-6, the sign of W kept (a zero magnitude included)

so that ``3 * 2^E < amax <= 6 * 2^E`` wherever E is not clamped: nothing saturates.  With E in [-13, 13] every non-zero
de-quantised value lies in [2^-14, 6 * 2^13]: a normal fp16 number and an exact bf16 number, so one quantiser serves both
dtypes and the 4-bit decode path is bit-identical to the 16-bit one on the de-quantised weights ("4-bit weights").

De-quantising and quantising again returns the same VALUES, always.  It returns the same ``(q, e)`` pair too, except for a
block whose largest element rounded to 3 (``amax / 2^E`` in (3, 3.5]): the de-quantised block has ``amax' = 3 * 2^E``, the
definition above then gives ``E - 1`` and elements twice as large ({0, 0.5, 1, 1.5, 2, 3} 2^E = {0, 1, 2, 3, 4, 6} 2^(E-1)) --
the same numbers, one exponent moved from the scale into the nibbles.  This is the 224 case of FP8.  (At the lower clamp the
exponent cannot move and the pair is unchanged, unless the whole block rounded to zero: then ``E`` becomes 0.)
"""
from __future__ import annotations

from typing import Tuple

import torch

E4M3_MAX = 448.0
MIN_SCALE_EXP = -120


def pow2_scale(amax: torch.Tensor) -> torch.Tensor:
    """``2^ceil(log2(amax / 448))`` for fp32 ``amax`` > 0 without a transcendental: amax = m 2^ex (m in [0.5, 1)),
    448 = 0.875 * 2^9, so the exponent is ex - 9, plus one when m > 0.875."""
    m, ex = torch.frexp(amax.float())
    e = (ex.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)).clamp_min(MIN_SCALE_EXP)
    return torch.ldexp(torch.ones_like(m), e)


def quantize_rows_e4m3(w: torch.Tensor, pow2: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """``w`` [N, K] (any float dtype) -> ``(q uint8 [N, K], scale fp32 [N])``."""
    if w.dim() != 2:
        raise ValueError("quantize_rows_e4m3: [N, K] weight expected")
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    safe = torch.where(amax > 0, amax, torch.ones_like(amax))
    scale = pow2_scale(safe) if pow2 else safe / E4M3_MAX
    scale = torch.where(amax > 0, scale, torch.ones_like(scale))
    # torch's cast does not saturate (500.0 becomes NaN): clamp first
    q = (wf / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, scale


def dequantize_rows_e4m3(q: torch.Tensor, scale: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``q`` uint8 [N, K], ``scale`` [N] -> ``q * scale`` in ``dtype`` (exact for power-of-two scales in fp16 / bf16)."""
    if q.dtype != torch.uint8 or q.dim() != 2 or scale.numel() != q.shape[0]:
        raise ValueError("dequantize_rows_e4m3: q uint8 [N, K] and scale [N] expected")
    return (q.view(torch.float8_e4m3fn).float() * scale.float()[:, None]).to(dtype)


# ---- OCP MX FP4 ------------------------------------------------------------------------------------------------------------
MX_BLOCK = 32
MX_EXP_MIN, MX_EXP_MAX = -13, 13
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mx_block_exp(amax: torch.Tensor) -> torch.Tensor:
    """``clamp(ceil(log2(amax / 6)), -13, 13)`` (int32) for fp32 ``amax`` >= 0 without a transcendental; 0 where amax == 0."""
    a = amax.float()
    m, ex = torch.frexp(torch.where(a > 0, a, torch.ones_like(a)))
    e = (ex.to(torch.int32) - 3 + (m > 0.75).to(torch.int32)).clamp(MX_EXP_MIN, MX_EXP_MAX)
    return torch.where(a > 0, e, torch.zeros_like(e))


def e2m1_rne(v: torch.Tensor) -> torch.Tensor:
    """fp32 -> e2m1 code 0..15 (uint8; bit 3 = the sign bit of ``v``): nearest, ties to the even mantissa bit, saturating."""
    a = v.abs().clamp(max=6.0)
    m, ex = torch.frexp(torch.where(a >= 1, a, torch.ones_like(a)))          # a = (2 m) 2^(ex - 1), 2 m in [1, 2)
    normal = 2 * ex.to(torch.int32) + torch.round((2 * m - 1) * 2).to(torch.int32)   # torch.round: half to even
    code = torch.where(a >= 1, normal, torch.round(a * 2).to(torch.int32))
    return (code + 8 * torch.signbit(v).to(torch.int32)).to(torch.uint8)


def quantize_blocks_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``w`` [N, K] (any float dtype, K % 32 == 0) -> ``(q uint8 [N, K/2], e uint8 [N, K/32])``."""
    if w.dim() != 2 or w.shape[1] % MX_BLOCK != 0 or w.shape[1] == 0:
        raise ValueError("quantize_blocks_mxfp4: [N, K] weight with K a multiple of 32 expected")
    N, K = w.shape
    wf = w.detach().float().view(N, K // MX_BLOCK, MX_BLOCK)
    ex = mx_block_exp(wf.abs().amax(dim=2))
    code = e2m1_rne(torch.ldexp(wf, -ex[:, :, None])).view(N, K // 2, 2)      # (a power-of-two division: exact)
    q = code[:, :, 0] | (code[:, :, 1] << 4)
    return q.contiguous(), (ex + 127).to(torch.uint8)


def dequantize_blocks_mxfp4(q: torch.Tensor, e: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``q`` uint8 [N, K/2], ``e`` uint8 [N, K/32] -> the [N, K] weight in ``dtype`` (exact in fp16 / bf16 for e in [114, 140])."""
    if q.dtype != torch.uint8 or e.dtype != torch.uint8 or q.dim() != 2 or e.dim() != 2 or q.shape[0] != e.shape[0] \
            or q.shape[1] != e.shape[1] * (MX_BLOCK // 2):
        raise ValueError("dequantize_blocks_mxfp4: q uint8 [N, K/2] and e uint8 [N, K/32] expected")
    N = q.shape[0]
    code = torch.stack([q & 15, q >> 4], dim=2).view(N, -1).to(torch.int64)
    mag = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=q.device)[code & 7]
    val = torch.where(code >= 8, -mag, mag).view(N, -1, MX_BLOCK)
    return torch.ldexp(val, (e.to(torch.int32) - 127)[:, :, None]).view(N, -1).to(dtype)
