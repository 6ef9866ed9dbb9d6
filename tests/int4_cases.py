"""AWQ and GPTQ packers written from the format descriptions in ops/int4.py, shared by the int4 tests."""
import torch

from rag_llm_k8s_amd.ops import int4 as I4


def _words(m, order=range(8)):
    """int [R, C] values 0..15 -> int32 [R, C/8]: nibble i of word c is column 8 c + order[i]."""
    m = m.long().reshape(m.shape[0], -1, 8)[:, :, list(order)]
    w = sum(m[:, :, i] << (4 * i) for i in range(8))
    return ((w + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


def pack_awq(codes, zeros, scales):
    """codes [N, K], zeros (0..15) / fp16 scales [N, K/G] -> qweight [K, N/8], qzeros [K/G, N/8], scales [K/G, N]."""
    return dict(qweight=_words(codes.t(), I4.AWQ_ORDER), qzeros=_words(zeros.t(), I4.AWQ_ORDER),
                scales=scales.t().contiguous())


def pack_gptq(codes, zeros, scales):
    """zeros 1..16, stored minus one -> qweight [K/8, N], qzeros [K/G, N/8], scales [K/G, N], g_idx [K]."""
    K, G = codes.shape[1], codes.shape[1] // zeros.shape[1]
    return dict(qweight=_words(codes).t().contiguous(), qzeros=_words(zeros.t() - 1), scales=scales.t().contiguous(),
                g_idx=(torch.arange(K) // G).int())


def random_params(N, K, seed, G=128, zlo=0, zhi=16, pow2=False):
    """codes [N, K], zeros in [zlo, zhi] and fp16 scales [N, K/G] (pow2: 2^-3..2^2, else around 0.01)."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    zeros = torch.randint(zlo, zhi + 1, (N, K // G), generator=g)
    if pow2:
        scales = torch.ldexp(torch.ones(N, K // G), torch.randint(-3, 3, (N, K // G), generator=g)).half()
    else:
        scales = (0.005 + 0.01 * torch.rand(N, K // G, generator=g)).half()
    return codes, zeros, scales
