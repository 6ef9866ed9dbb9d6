"""fp8 (OCP e4m3fn) weights: container, quantization and the fp32 reference (BASELINE config 5).

A linear layer's bf16 weight W [rows, K] is stored as W8 (e4m3fn) with one fp32 scale per
row, W ≈ W8 * s[:, None], s = amax|W[row]| / 448. Rows keep their bf16 order, so the packed
gate/up layout and fused qkv rows carry over unchanged. On the GPU:
  * decode (M <= 64)  W8A16 -- weights streamed at 1 byte each, dequantized exactly to bf16
                      in registers (csrc/kernels/gemm_fp8.hip, gemm_fp8_dec);
  * prefill (M > 64)  W8A8  -- activations quantized per token (quant_rows) and multiplied
                      with the block-scaled fp8 MFMA (gemm_fp8_tile).
`reference_linear` reproduces exactly that arithmetic in fp32 (the oracle of the GPU tests and
the CPU path).

The opt-in fp8 KV cache (`Fp8KV`, KV_CACHE_DTYPE=fp8) reuses the activation quantization: a cached k / v row is
`quantize_rows` of the bf16 row, on every write path of both backends (csrc/kernels/kv_fp8.h on the GPU).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import reference as R

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
DEC_MAX_M = 64


@dataclass
class Fp8Weight:
    w8: torch.Tensor  # float8_e4m3fn [rows, K]
    scale: torch.Tensor  # fp32 [rows]

    @property
    def shape(self):
        return self.w8.shape

    @property
    def device(self):
        return self.w8.device

    def dequant(self, dtype=torch.float32):
        return (self.w8.float() * self.scale[:, None]).to(dtype)

    def nbytes(self):
        return self.w8.numel() + 4 * self.scale.numel()


@dataclass
class Fp8KV:
    """One side (K or V) of an fp8 paged KV cache: `data` [nblocks, Hkv, 64, D] e4m3fn and one fp32 `scale` per
    cached row [nblocks, Hkv, 64]; a row x is stored as quantize_rows(x), x ~= data * scale[..., None]. Every
    writer (GPU or CPU) produces exactly quantize_rows of the bf16 value the bf16 cache would hold."""
    data: torch.Tensor
    scale: torch.Tensor

    @property
    def shape(self):
        return self.data.shape

    @property
    def device(self):
        return self.data.device

    @property
    def dtype(self):
        return self.data.dtype

    def dequant(self, dtype=torch.float32):
        return (self.data.float() * self.scale[..., None]).to(dtype)

    def nbytes(self):
        return self.data.numel() + 4 * self.scale.numel()

    def write_rows(self, blocks, offs, rows):
        """rows [n, Hkv, D] (bf16 values) -> cache rows (blocks[i], :, offs[i]), quantized per (token, head)."""
        n, Hkv, D = rows.shape
        q, s = quantize_rows(rows.reshape(n * Hkv, D))
        self.data.view(torch.uint8)[blocks, :, offs] = q.view(torch.uint8).view(n, Hkv, D)  # bytes: no fp8 index_put
        self.scale[blocks, :, offs] = s.view(n, Hkv)


def alloc_fp8_kv(num_blocks, Hkv, block, D, device):
    return Fp8KV(torch.zeros((num_blocks, Hkv, block, D), dtype=torch.uint8, device=device).view(FP8),
                 torch.ones((num_blocks, Hkv, block), dtype=torch.float32, device=device))


KV_CACHE_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp8": FP8, "fp8_e4m3": FP8}


def kv_cache_torch_dtype(dtype):
    """"bf16" | "fp8" (or a torch dtype) -> the KV cache's torch dtype; anything else is an error."""
    if isinstance(dtype, torch.dtype):
        return dtype
    try:
        return KV_CACHE_DTYPES[str(dtype).strip().lower()]
    except KeyError:
        raise ValueError("kv cache dtype must be 'bf16' or 'fp8', got %r" % (dtype,)) from None


def kv_cache_dtype_name(dtype):
    return "fp8" if kv_cache_torch_dtype(dtype) == FP8 else "bf16"


def check_fp8_kv_head_dim(D, what="this model"):
    """The fp8 KV cache kernels are built for head_dim 128 only: refuse instead of falling back to bf16."""
    if D != 128:
        raise ValueError("fp8 KV cache needs head_dim 128; %s has head_dim %d (use kv_cache_dtype=bf16)" % (what, D))


def quantize_weight(w: torch.Tensor) -> Fp8Weight:
    """Per-output-row symmetric e4m3fn quantization (round to nearest even, no saturation needed:
    every |w / s| <= 448)."""
    wf = w.float()
    s = wf.abs().amax(dim=1).clamp_min(1e-12) / FP8_MAX
    w8 = (wf / s[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return Fp8Weight(w8.contiguous(), s.contiguous())


def quantize_rows(x: torch.Tensor):
    """Dynamic per-row activation quantization, as the GPU quant_rows kernel does."""
    xf = x.float()
    a = xf.abs().amax(dim=1)
    s = torch.where(a > 0, a * torch.tensor(1.0 / FP8_MAX, dtype=torch.float32), torch.ones_like(a))
    inv = torch.ones_like(s) / s  # correctly rounded, like the kernel's __fdiv_rn
    q = (xf * inv[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return q, s


def reference_linear(x, w: Fp8Weight, bias=None, resid=None, epi="none", out_f32=False):
    """fp32 oracle of ragk_gemm_fp8: W8A16 for M <= 64, W8A8 above."""
    wd = w.dequant()
    if x.shape[0] <= DEC_MAX_M:
        xe = x.float()
    else:
        q, s = quantize_rows(x)
        xe = q.float() * s[:, None]
    y = R.linear(xe, wd, bias, resid, epi=epi, out_f32=True)
    return y if out_f32 else y.to(x.dtype)
