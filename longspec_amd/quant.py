"""Row-wise FP8 (OCP e4m3fn) weight quantisation on the host -- pure torch, runs on CPU.

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
