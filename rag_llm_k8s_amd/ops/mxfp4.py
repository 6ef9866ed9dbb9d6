"""OCP MXFP4 weights: container, quantizer and the fp32 reference of the GPU kernels (opt-in, DTYPE=mxfp4).

A linear layer's bf16 weight W [rows, K] is stored as e2m1 elements, two per byte, with one E8M0
scale byte per row and per 32 consecutive k: 4.25 bits per weight.
  * nibble code: bit 3 is the sign, bits 2..0 index the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6;
  * element k sits in the low nibble of byte k // 2 when k is even, in the high nibble when odd;
  * W[n, k] = LUT[code] * 2^(scale[n, k // 32] - 127), exact in bf16.
Rows keep their bf16 order, so the packed gate/up layout and fused qkv rows carry over unchanged. On the GPU
(csrc/kernels/gemm_mxfp4.hip):
  * decode (M <= 64)  W4A16 -- weights dequantized exactly to bf16 in registers, bf16 MFMA against the
                      unquantized activations (gemm_mxfp4_dec);
  * prefill (M > 64)  W4A8  -- activations quantized per token (ops/fp8.quantize_rows) and multiplied with
                      the block-scaled e4m3 x e2m1 MFMA (gemm_mxfp4_tile).
`reference_linear` reproduces exactly that arithmetic in fp32 (the oracle of the GPU tests and the CPU path).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import reference as R
from .fp8 import DEC_MAX_M, quantize_rows

BLOCK = 32  # elements per scale
E2M1_LUT = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _lut(device):
    mags = torch.tensor(E2M1_LUT, dtype=torch.float32, device=device)
    return torch.cat([mags, -mags])


@dataclass
class Mxfp4Weight:
    packed: torch.Tensor  # uint8 [rows, K/2]
    scale: torch.Tensor  # uint8 [rows, K/32], E8M0 exponent bytes (1..254)

    @property
    def shape(self):
        return torch.Size((self.packed.shape[0], 2 * self.packed.shape[1]))

    @property
    def device(self):
        return self.packed.device

    def codes(self):
        """uint8 [rows, K] nibble codes in k order."""
        p = self.packed
        return torch.stack([p & 0xF, p >> 4], dim=2).reshape(p.shape[0], 2 * p.shape[1])

    def dequant(self, dtype=torch.float32):
        rows, K = self.shape
        v = _lut(self.device)[self.codes().long()]
        e = (self.scale.to(torch.int32) - 127).repeat_interleave(BLOCK, dim=1)
        # ldexp in two halves: 2^-127 alone underflows to an fp32 subnormal before the multiply
        h = e // 2
        w = torch.ldexp(torch.ldexp(v, h), e - h)
        return w.to(dtype)

    def nbytes(self):
        return self.packed.numel() + self.scale.numel()


def quantize_weight(w: torch.Tensor) -> Mxfp4Weight:
    """OCP MX quantization per row and per 32 consecutive k: shared exponent e = floor(log2(amax)) - 2
    clamped to [-126, 127] (an all-zero block: e = 0), elements w / 2^e rounded to nearest even on the e2m1
    grid and saturated at +-6. Quantizing dequant(q) again gives q back."""
    if w.dim() != 2 or w.shape[1] % 128:
        raise ValueError("mxfp4 weights need a 2-D weight with K %% 128 == 0, got shape %s" % (tuple(w.shape),))
    rows, K = w.shape
    wf = w.float().reshape(rows, K // BLOCK, BLOCK)
    amax = wf.abs().amax(dim=2)
    _, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, (ex - 3).clamp(-126, 127), torch.zeros_like(ex)).to(torch.int32)
    h = e // 2
    v = torch.ldexp(torch.ldexp(wf, -h[..., None]), -(e - h)[..., None])  # exact scaling by 2^-e
    a = v.abs().clamp(max=6.0)
    # round to nearest even on the grid: step 0.5 below 2, 1 in [2, 4), 2 above (torch.round is half-to-even,
    # and the even neighbour of every tie is the code with mantissa bit 0)
    m = torch.where(a < 2.0, torch.round(a * 2.0) * 0.5, torch.where(a < 4.0, torch.round(a), torch.round(a * 0.5) * 2.0))
    code = torch.where(m <= 2.0, m * 2.0, torch.where(m <= 4.0, m + 2.0, torch.full_like(m, 7.0))).to(torch.uint8)
    code = code | (torch.signbit(v).to(torch.uint8) << 3)
    code = code.reshape(rows, K // 2, 2)
    packed = code[:, :, 0] | (code[:, :, 1] << 4)
    return Mxfp4Weight(packed.contiguous(), (e + 127).to(torch.uint8).contiguous())


def reference_linear(x, w: Mxfp4Weight, bias=None, resid=None, epi="none", out_f32=False):
    """fp32 oracle of ragk_gemm_mxfp4: W4A16 for M <= 64, W4A8 above."""
    wd = w.dequant()
    if x.shape[0] <= DEC_MAX_M:
        xe = x.float()
    else:
        q, s = quantize_rows(x)
        xe = q.float() * s[:, None]
    y = R.linear(xe, wd, bias, resid, epi=epi, out_f32=True)
    return y if out_f32 else y.to(x.dtype)
