"""4-bit integer weights (AWQ / GPTQ checkpoints): container, quantizer, checkpoint unpackers and the fp32
reference of the GPU kernels (opt-in, DTYPE=int4).

A linear layer's weight W [rows, K] is stored as 4-bit codes with one zero point and one fp16 scale per row and
per 128 consecutive k: 4.25 bits per weight.
  * W[n, k] = scale[n, k // 128] * (code[n, k] - zero[n, k // 128]), code 0..15, zero 0..16;
  * `meta` int32 [rows, K/128]: bits 0..15 the fp16 scale, bits 16..20 the zero point;
  * `packed` uint8 [rows, K/2]: of each 8 consecutive k (one dword), byte j holds code k0 + j in its low nibble
    and code k0 + 4 + j in its high nibble, j = 0..3. So `d & 0x0f0f0f0f` is codes k0..k0+3 and
    `(d >> 4) & 0x0f0f0f0f` codes k0+4..k0+7, one per byte in k order: the kernel converts a byte to fp32 with
    one v_cvt_f32_ubyte and packs neighbours to a bf16 pair.
Rows keep their bf16 order, so the packed gate/up layout and fused qkv rows carry over unchanged. On the GPU
(csrc/kernels/gemm_int4.hip):
  * M <= 64  W4A16 -- the exact integers code - zero as bf16 against the unquantized activations, each 128-deep
             K block into its own fp32 accumulator, folded in as acc += fp32(scale) * part (gemm_int4_dec);
  * M > 64   dequant_int4 writes bf16_rne(fp32(scale) * (code - zero)) into a scratch and the bf16 GEMM runs.
`reference_linear` is the fp32 oracle of both routes and the CPU path.

The group size is 128: one MFMA chain sums over a 128-deep K block, so a finer scale cannot be applied after
it. Per-channel checkpoints repeat their meta word per 128.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import reference as R
from .fp8 import DEC_MAX_M

GROUP = 128  # weights per (scale, zero)
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)  # AutoAWQ gemm: nibble i of a word is column 8 c + AWQ_ORDER[i]


def make_meta(scale: torch.Tensor, zero: torch.Tensor) -> torch.Tensor:
    """fp16 scale, integer zero 0..16 (same shape) -> int32 meta words."""
    s = scale.to(torch.float16).contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return (s | (zero.to(torch.int32) << 16)).contiguous()


def pack_codes(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes [rows, K] in k order -> packed [rows, K/2] (nibble order: module docstring)."""
    rows, K = codes.shape
    c = codes.to(torch.uint8).reshape(rows, K // 8, 2, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 4)).reshape(rows, K // 2).contiguous()


@dataclass
class Int4Weight:
    packed: torch.Tensor  # uint8 [rows, K/2]
    meta: torch.Tensor  # int32 [rows, K/128]: fp16 scale | zero << 16

    @property
    def shape(self):
        return torch.Size((self.packed.shape[0], 2 * self.packed.shape[1]))

    @property
    def device(self):
        return self.packed.device

    @classmethod
    def from_codes(cls, codes, scale, zero):
        """codes [rows, K] 0..15, scale fp16 / zero 0..16 [rows, K/128]."""
        return cls(pack_codes(codes), make_meta(scale, zero))

    def codes(self):
        """uint8 [rows, K] codes in k order."""
        p = self.packed.reshape(self.packed.shape[0], -1, 1, 4)
        return torch.cat([p & 0xF, p >> 4], dim=2).reshape(self.shape)

    def scales(self):
        return self.meta.contiguous().view(torch.int16)[:, 0::2].contiguous().view(torch.float16)  # low halves

    def zeros(self):
        return (self.meta >> 16) & 0x1F

    def dequant(self, dtype=torch.float32):
        """fp32(scale) * (code - zero): exact in fp32 (11 x 5 significant bits), rounded once to `dtype`."""
        d = self.codes().to(torch.int32) - self.zeros().repeat_interleave(GROUP, dim=1)
        return (self.scales().float().repeat_interleave(GROUP, dim=1) * d.float()).to(dtype)

    def nbytes(self):
        return self.packed.numel() + 4 * self.meta.numel()

    def cat_rows(self, *others):
        ws = (self,) + others
        return Int4Weight(torch.cat([w.packed for w in ws], 0), torch.cat([w.meta for w in ws], 0))

    def slice(self, rows=None, cols=None):
        """Row range and / or K range (a multiple of 128: the row-parallel TP shard)."""
        p, m = self.packed, self.meta
        if rows is not None:
            p, m = p[rows[0]:rows[1]], m[rows[0]:rows[1]]
        if cols is not None:
            if cols[0] % GROUP or cols[1] % GROUP:
                raise ValueError("int4 weights shard K in multiples of %d, got %s" % (GROUP, (cols,)))
            p, m = p[:, cols[0] // 2:cols[1] // 2], m[:, cols[0] // GROUP:cols[1] // GROUP]
        return Int4Weight(p.contiguous(), m.contiguous())

    def to(self, device):
        return Int4Weight(self.packed.to(device), self.meta.to(device))


def quantize_weight(w: torch.Tensor) -> Int4Weight:
    """Round to nearest, asymmetric, per row and per 128 k: scale = fp16((max - min) / 15) (an all-equal group:
    1), zero = clamp(round(-min / scale), 0, 15), code = clamp(round(w / scale) + zero, 0, 15). A group whose
    codes span 0..15 quantizes to itself again."""
    if w.dim() != 2 or w.shape[1] % GROUP:
        raise ValueError("int4 weights need a 2-D weight with K %% 128 == 0, got shape %s" % (tuple(w.shape),))
    rows, K = w.shape
    wf = w.float().reshape(rows, K // GROUP, GROUP)
    mn, mx = wf.amin(dim=2), wf.amax(dim=2)
    s = ((mx - mn) / 15.0).clamp(max=65504.0).to(torch.float16)
    s = torch.where(s.float() > 0, s, torch.ones_like(s))  # all-equal (or a range below fp16): scale 1
    sf = s.float()
    zero = torch.round(-mn / sf).clamp(0, 15)
    code = (torch.round(wf / sf[..., None]) + zero[..., None]).clamp(0, 15)
    return Int4Weight.from_codes(code.reshape(rows, K).to(torch.uint8), s, zero)


def reference_linear(x, w: Int4Weight, bias=None, resid=None, epi="none", out_f32=False):
    """fp32 oracle of the two GPU routes: M <= 64 multiplies by the unrounded fp32 dequantization, above that
    by the bf16 scratch dequant_int4 writes."""
    if x.shape[0] <= DEC_MAX_M:
        y = R.linear(x.float(), w.dequant(torch.float32), bias, resid, epi=epi, out_f32=True)
        return y if out_f32 else y.to(x.dtype)
    return R.linear(x, w.dequant(torch.bfloat16), bias, resid, epi=epi, out_f32=out_f32)


# ------------------------------------------------------------------------------------- checkpoint formats
def check_quant_config(qc: dict, K=None):
    """Validate an HF `quantization_config` of an AWQ / GPTQ checkpoint; returns 'awq' or 'gptq'. Everything this
    server has no kernel for is refused with the reason."""
    method = str(qc.get("quant_method", "")).lower()
    if method not in ("awq", "gptq"):
        raise ValueError("DTYPE=int4 loads quant_method awq or gptq checkpoints, got %r" % qc.get("quant_method"))
    bits = qc.get("bits", qc.get("w_bit"))
    if bits != 4:
        raise ValueError("DTYPE=int4 needs a 4-bit checkpoint, this one has bits=%r" % (bits,))
    check_group_size(qc.get("group_size", qc.get("q_group_size", GROUP)), K)
    if method == "awq":
        if str(qc.get("version", "gemm")).lower() != "gemm":
            raise ValueError("AWQ version %r: only the 'gemm' packing is supported" % qc.get("version"))
        if not qc.get("zero_point", True):
            raise ValueError("AWQ checkpoints without zero points (zero_point: false) are not supported")
    else:
        if qc.get("desc_act", False):
            raise ValueError("GPTQ desc_act: true permutes the groups along K (g_idx); the int4 kernels need "
                             "consecutive groups of 128 -- re-export the checkpoint with desc_act: false")
        if str(qc.get("checkpoint_format", "gptq")).lower() not in ("gptq", "v1"):
            raise ValueError("GPTQ checkpoint_format %r: only v1 ('gptq', zeros stored minus one) is supported"
                             % qc.get("checkpoint_format"))
    return method


def check_group_size(g, K=None):
    if g in (GROUP, -1) or (K is not None and g == K):
        return
    raise ValueError("int4 group_size %r: the kernels apply one scale per 128-deep MFMA K block, so only "
                     "group_size 128 or per-channel (-1 / K) checkpoints load" % (g,))


def _nibbles(q, order=None):
    """int32 [..., C] -> uint8 [..., 8 C]: nibble i of word c is element 8 c + order[i]."""
    n = torch.stack([(q >> (4 * i)) & 0xF for i in range(8)], dim=-1)
    if order is not None:
        out = torch.empty_like(n)
        out[..., list(order)] = n
        n = out
    return n.reshape(*q.shape[:-1], q.shape[-1] * 8).to(torch.uint8)


def _finish(codes_kn, zeros_gn, scales_gn, k_range):
    """codes [K, N], zeros / scales [K/G, N] (G = 128 or K) -> Int4Weight of rows N over the K range."""
    K, N = codes_kn.shape
    groups = scales_gn.shape[0]
    if scales_gn.dtype != torch.float16 or zeros_gn.shape != scales_gn.shape or K % GROUP:
        raise ValueError("int4 checkpoint tensors: fp16 scales and zeros [K/G, N] with K %% 128 == 0 expected")
    if groups == 1:  # per-channel: the meta word repeats per 128
        zeros_gn, scales_gn = zeros_gn.expand(K // GROUP, N), scales_gn.expand(K // GROUP, N)
    elif groups * GROUP != K:
        check_group_size(K // groups, K)
    lo, hi = k_range if k_range is not None else (0, K)
    if lo % GROUP or hi % GROUP:
        raise ValueError("int4 weights shard K in multiples of %d, got %s" % (GROUP, (k_range,)))
    return Int4Weight.from_codes(codes_kn[lo:hi].t().contiguous(), scales_gn[lo // GROUP:hi // GROUP].t(),
                                 zeros_gn[lo // GROUP:hi // GROUP].t())


def unpack_awq(qweight, qzeros, scales, k_range=None) -> Int4Weight:
    """AutoAWQ 'gemm': qweight int32 [K, N/8], qzeros int32 [K/G, N/8], scales fp16 [K/G, N];
    W[k, n] = (q - z) * s."""
    return _finish(_nibbles(qweight, AWQ_ORDER), _nibbles(qzeros, AWQ_ORDER), scales, k_range)


def unpack_gptq(qweight, qzeros, scales, g_idx=None, k_range=None) -> Int4Weight:
    """AutoGPTQ v1, desc_act false: qweight int32 [K/8, N] (nibble i of word [r, n] is k = 8 r + i), qzeros
    int32 [K/G, N/8] storing zero - 1, scales fp16 [K/G, N]."""
    K = qweight.shape[0] * 8
    codes = _nibbles(qweight.t().contiguous()).t()  # [K, N]
    if g_idx is not None:
        G = K // scales.shape[0]
        if not torch.equal(g_idx.long().cpu(), torch.arange(K) // G):
            raise ValueError("GPTQ g_idx is not k // group_size (an act-order checkpoint): not supported")
    return _finish(codes, _nibbles(qzeros).to(torch.int32) + 1, scales, k_range)
