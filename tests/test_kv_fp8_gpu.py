"""fp8 KV cache on the GPU (csrc/kernels/kv_fp8.h): the quantizing cache writes bit for bit against
quantize_rows of the bf16 cache, the fp8 attention kernels against the fp32 oracle over the dequantized cache,
and the engine end to end. Every fp8 write / attention call runs on sentinel-padded outputs, caches and scale
arrays (as tests/test_canary_gpu.py), which must be intact afterwards.

Test data: D = 128; K rows scaled by 2^U(-3,1) and V rows by 2^U(-4,4) per row (a dropped, swapped or
misindexed scale fails); one all-zero K row and one all-zero V row inside kv_len (the s = 1 branch); every slot
of every allocated block holds finite random data (tails past kv_len are live garbage); permuted block tables."""
import itertools
import math

import pytest
import torch

from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams
from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, StepInput, llama_tiny
from rag_llm_k8s_amd.ops import reference as R
from rag_llm_k8s_amd.ops.backend import AttnMeta
from rag_llm_k8s_amd.ops.fp8 import FP8, Fp8KV, quantize_rows
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
PAD = 4096  # sentinel elements on each side of a guarded allocation
BYTE_SENT, F32_SENT, BF_SENT = 0x5A, -7.0, -7.0


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


class Guard:
    """Views into larger allocations whose heads and tails hold a sentinel."""

    def __init__(self):
        self.bufs = []

    def alloc(self, shape, dtype, sentinel):
        n = math.prod(shape)
        buf = torch.full((2 * PAD + n,), sentinel, dtype=dtype, device=DEV)
        self.bufs.append((buf, sentinel))
        return buf[PAD:PAD + n].view(*shape)

    def fp8_cache(self, c: Fp8KV):
        """A guarded GPU copy of a CPU Fp8KV."""
        d = self.alloc(tuple(c.data.shape), torch.uint8, BYTE_SENT)
        d.copy_(c.data.view(torch.uint8))
        s = self.alloc(tuple(c.scale.shape), torch.float32, F32_SENT)
        s.copy_(c.scale)
        return Fp8KV(d.view(FP8), s)

    def out(self, shape, fill=float("nan")):
        o = self.alloc(shape, torch.bfloat16, BF_SENT)
        o.fill_(fill)
        return o

    def intact(self):
        torch.cuda.synchronize()
        for buf, sent in self.bufs:
            s = torch.tensor(sent, dtype=buf.dtype)
            if not (bool(buf[:PAD].cpu().eq(s).all()) and bool(buf[-PAD:].cpu().eq(s).all())):
                return False
        return True


def _rows(n, lo, hi, g):
    """n rows of D normal values, row i scaled by 2^U(lo, hi), as bf16."""
    return (torch.randn(n, D, generator=g) * torch.exp2(torch.empty(n, 1).uniform_(lo, hi, generator=g))).bfloat16()


def _paged_fp8(lens, Hkv, seed=0):
    """(k16, v16, K8, V8, block_tables) on the CPU: bf16 caches filled everywhere with finite rows (the issue's
    scales), one zero K row and one zero V row inside sequence 0, and their quantize_rows forms."""
    g = torch.Generator().manual_seed(seed)
    nb_per = [(L + 63) // 64 for L in lens]
    total = sum(nb_per) + 3
    k16 = _rows(total * Hkv * 64, -3, 1, g).view(total, Hkv, 64, D)
    v16 = _rows(total * Hkv * 64, -4, 4, g).view(total, Hkv, 64, D)
    perm = torch.randperm(total, generator=g)
    bt = torch.zeros(len(lens), max(nb_per), dtype=torch.int32)
    i = 0
    for s, nb in enumerate(nb_per):
        bt[s, :nb] = perm[i:i + nb].int()
        i += nb
    zk, zv = min(lens[0] - 1, 3), (lens[0] - 1) // 2  # positions of the all-zero rows (sequence 0, KV head 0)
    k16[int(bt[0, zk // 64]), 0, zk % 64] = 0
    v16[int(bt[0, zv // 64]), 0, zv % 64] = 0
    return k16, v16, _quant(k16), _quant(v16), bt


def _quant(c16):
    q, s = quantize_rows(c16.reshape(-1, D))
    return Fp8KV(q.view(c16.shape), s.view(c16.shape[:3]))


def _same(a: Fp8KV, b: Fp8KV):
    return (torch.equal(a.data.view(torch.uint8).cpu(), b.data.view(torch.uint8).cpu())
            and torch.equal(a.scale.cpu(), b.scale.cpu()))


def _oracle(q, K8, V8, bt, kv_lens, cu_q, Hq):
    """fp32 attention over the dequantized cache (queries = the last q_len positions of each context)."""
    kd, vd = K8.dequant().cpu(), V8.dequant().cpu()
    btc = bt.cpu()
    return R.attention_varlen(q.cpu().reshape(-1, Hq, D), None, None, cu_q, kv_lens, True, 1 / math.sqrt(D),
                              k_full=lambda s: R.paged_kv_view(kd, btc[s], kv_lens[s], 64),
                              v_full=lambda s: R.paged_kv_view(vd, btc[s], kv_lens[s], 64))


def _rope(maxpos=8192):
    cos, sin = R.rope_tables(D, maxpos, theta=500000.0)
    return cos.to(DEV), sin.to(DEV)


# ------------------------------------------------------------------------------------- 1. write paths
def _expected_after_write(K8_0: Fp8KV, k16_after, slots):
    """The initial fp8 cache with the rows at `slots` (>= 0, all KV heads) replaced by quantize_rows of the bf16
    cache after the same write: untouched rows must stay untouched."""
    exp = Fp8KV(K8_0.data.clone(), K8_0.scale.clone())
    want = _quant(k16_after.cpu())
    s = slots.cpu().long()
    s = s[s >= 0]
    exp.data.view(torch.uint8)[s // 64, :, s % 64] = want.data.view(torch.uint8)[s // 64, :, s % 64]
    exp.scale[s // 64, :, s % 64] = want.scale[s // 64, :, s % 64]
    return exp


@pytest.mark.parametrize("partials", [False, True])
def test_rope_kv_fp8_writes_quantize_rows_of_bf16(native, partials):
    """rope_kv / rope_kv_partials: T = 70 tokens across a block boundary, some slots = -1, (Hq, Hkv) = (8, 2)."""
    Hq, Hkv, T, S = 8, 2, 70, 3
    k16, v16, K8, V8, bt = _paged_fp8([200], Hkv, seed=1)
    gd = Guard()
    K8g, V8g = gd.fp8_cache(K8), gd.fp8_cache(V8)
    k16g, v16g = k16.to(DEV), v16.to(DEV)
    g = torch.Generator().manual_seed(2)
    pos = torch.arange(50, 50 + T)
    slots = (bt[0, pos // 64].long() * 64 + pos % 64).int()
    slots[[3, 17, 69]] = -1
    width = (Hq + 2 * Hkv) * D
    cos, sin = _rope()
    posg, slotsg = pos.int().to(DEV), slots.to(DEV)
    if partials:
        P = torch.randn(S, T, width, generator=g).to(DEV)
        qa = gd.out((T, Hq * D))
        qb = torch.empty(T, Hq * D, device=DEV).bfloat16()
        native.rope_kv_partials(P, qb, posg, cos, sin, slotsg, k16g, v16g, Hq, Hkv, D)
        native.rope_kv_partials(P, qa, posg, cos, sin, slotsg, K8g, V8g, Hq, Hkv, D)
    else:
        qkv = torch.randn(T, width, generator=g).bfloat16()
        qb = qkv.to(DEV)
        qa = gd.out((T, width))
        qa.copy_(qkv)
        native.rope_kv(qb, posg, cos, sin, slotsg, k16g, v16g, Hq, Hkv, D)
        native.rope_kv(qa, posg, cos, sin, slotsg, K8g, V8g, Hq, Hkv, D)
    assert gd.intact()
    assert torch.equal(qa, qb)  # rotated q (and k in place) do not depend on the cache format
    assert _same(K8g, _expected_after_write(K8, k16g, slots))
    assert _same(V8g, _expected_after_write(V8, v16g, slots))
    assert not _same(K8g, K8)


def _decode_setup(kv_lens, Hq, Hkv, seed, S=4):
    k16, v16, K8, V8, bt = _paged_fp8(kv_lens, Hkv, seed=seed)
    B = len(kv_lens)
    btg = bt.to(DEV)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    pos = kvl - 1
    slots = (btg[torch.arange(B, device=DEV), (pos // 64).long()] * 64 + pos % 64).int()
    g = torch.Generator().manual_seed(seed + 100)
    P = torch.randn(S, B, (Hq + 2 * Hkv) * D, generator=g).to(DEV)
    return k16, v16, K8, V8, btg, kvl, pos, slots, P


@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (4, 1), (8, 1)])
def test_decode_append_fp8_writes_quantize_rows_of_bf16(native, Hq, Hkv):
    """The fused append of attn_decode_rope: new tokens at a block end, a block start and alone."""
    kv_lens = [64, 65, 1, 321]
    k16, v16, K8, V8, bt, kvl, pos, slots, P = _decode_setup(kv_lens, Hq, Hkv, seed=3)
    gd = Guard()
    K8g, V8g = gd.fp8_cache(K8), gd.fp8_cache(V8)
    k16g, v16g = k16.to(DEV), v16.to(DEV)
    cos, sin = _rope()
    B = len(kv_lens)
    pt, mp = native.decode_partitions(max(kv_lens), B, Hkv, target_blocks=64)
    out16 = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.attn_decode_rope(P, pos, cos, sin, slots, k16g, v16g, bt, kvl, out16, Hq, Hkv, D, pt, mp)
    out8 = gd.out((B, Hq * D))
    native.attn_decode_rope(P, pos, cos, sin, slots, K8g, V8g, bt, kvl, out8, Hq, Hkv, D, pt, mp)
    assert gd.intact()
    assert _same(K8g, _expected_after_write(K8, k16g, slots))
    assert _same(V8g, _expected_after_write(V8, v16g, slots))
    assert bool(torch.isfinite(out8.float()).all())


# ------------------------------------------------------------------------------------- 2. decode attention
KV_SETS = [[1], [64, 65, 1, 129], [700, 5, 321]]


def _check_decode(native, kv_lens, Hq, Hkv, pt, mp, seed):
    k16, v16, K8, V8, bt = _paged_fp8(kv_lens, Hkv, seed=seed)
    B = len(kv_lens)
    gd = Guard()
    K8g, V8g = gd.fp8_cache(K8), gd.fp8_cache(V8)
    q = torch.randn(B, Hq * D, generator=torch.Generator().manual_seed(seed + 1)).bfloat16()
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    out = gd.out((B, Hq * D))
    native.attn_decode(q.to(DEV), K8g, V8g, bt.to(DEV), kvl.to(DEV), out, Hq, Hkv, D, pt, mp)
    assert gd.intact()
    assert _same(K8g, K8) and _same(V8g, V8)
    ref = _oracle(q, K8, V8, bt, kv_lens, torch.arange(B + 1, dtype=torch.int32), Hq)
    e = rel_err(out.cpu().reshape(B, Hq, D), ref)
    print("decode fp8 rel_err %.3e" % e)
    assert e < 2e-2, e


@pytest.mark.parametrize("target", [8, 1024])
@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (8, 1), (4, 1), (4, 2), (2, 2)])
@pytest.mark.parametrize("kv_lens", KV_SETS)
def test_attn_decode_fp8_split_k(native, kv_lens, Hq, Hkv, target):
    """Split-K route, G in {4, 8, 4, 2, 1}; few and many partitions (partitions past a short context exit early)."""
    pt, mp = native.decode_partitions(max(kv_lens), len(kv_lens), Hkv, target_blocks=target)
    _check_decode(native, kv_lens, Hq, Hkv, pt, mp, seed=11)


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (4, 1)])
@pytest.mark.parametrize("kv_lens", KV_SETS)
def test_attn_decode_fp8_single_partition(native, kv_lens, Hq, Hkv, nt, monkeypatch):
    """The batch-32 route (one 4-wave block per sequence and KV head, K tiles by LDS-DMA), nt loads on and off."""
    monkeypatch.setattr(native, "DECODE_NW8_MIN_PAIRS", 1)
    monkeypatch.setattr(native, "DECODE_NT_MIN_BH", 1 if nt else 1 << 30)
    pt, mp = native.decode_partitions(max(kv_lens), len(kv_lens), Hkv)
    assert mp == 1 and native.DECODE_KL
    _check_decode(native, kv_lens, Hq, Hkv, pt, mp, seed=12)


# ------------------------------------------------------------------------------------- 3. fused == unfused
@pytest.mark.parametrize("route,Hq,Hkv", [("split", 32, 8), ("split", 4, 1), ("split", 8, 1),
                                          ("single", 32, 8), ("single", 4, 1)])  # single: 4 query heads per KV head
def test_attn_decode_rope_fp8_matches_unfused(native, Hq, Hkv, route, monkeypatch):
    """attn_decode_rope (fp8) == rope_kv_partials (fp8) + attn_decode (fp8): the cache bit for bit; the output
    bit for bit on the split-K route, within 1e-2 on the single-partition (K by LDS-DMA) route -- the assertions
    of the bf16 pair tests."""
    if route == "single":
        monkeypatch.setattr(native, "DECODE_NW8_MIN_PAIRS", 1)
        monkeypatch.setattr(native, "DECODE_NT_MIN_BH", 1)
    kv_lens = [64, 65, 1, 321, 700]
    k16, v16, K8, V8, bt, kvl, pos, slots, P = _decode_setup(kv_lens, Hq, Hkv, seed=5, S=8)
    B = len(kv_lens)
    gd = Guard()
    Ka, Va, Kb, Vb = gd.fp8_cache(K8), gd.fp8_cache(V8), gd.fp8_cache(K8), gd.fp8_cache(V8)
    cos, sin = _rope()
    pt, mp = native.decode_partitions(max(kv_lens), B, Hkv, target_blocks=64)
    assert (mp == 1) == (route == "single")
    q = gd.out((B, Hq * D))
    ref = gd.out((B, Hq * D))
    native.rope_kv_partials(P, q, pos, cos, sin, slots, Kb, Vb, Hq, Hkv, D)
    native.attn_decode(q, Kb, Vb, bt, kvl, ref, Hq, Hkv, D, pt, mp)
    out = gd.out((B, Hq * D))
    native.attn_decode_rope(P, pos, cos, sin, slots, Ka, Va, bt, kvl, out, Hq, Hkv, D, pt, mp)
    assert gd.intact()
    assert _same(Ka, Kb) and _same(Va, Vb) and not _same(Ka, K8)
    if route == "single":
        assert rel_err(out, ref) < 1e-2
    else:
        assert torch.equal(out, ref)
    # and against the oracle over the appended, dequantized cache
    Kc, Vc = Fp8KV(Ka.data.cpu(), Ka.scale.cpu()), Fp8KV(Va.data.cpu(), Va.scale.cpu())
    oracle = _oracle(q, Kc, Vc, bt, kv_lens, torch.arange(B + 1, dtype=torch.int32), Hq)
    assert rel_err(out.cpu().reshape(B, Hq, D), oracle) < 2e-2


def test_gemm_part_merge_fp8_cache_matches_reduce_then_part(native):
    """defer_merge at B = 2: the o_proj GEMM merging the unmerged fp8-cache partitions (gemm_part_merge) against
    attn_decode_rope (reduce launch) + gemm_part, with the tolerances of the bf16 merge test."""
    Hq, Hkv = 32, 8
    kv_lens = [700, 321]
    k16, v16, K8, V8, bt, kvl, pos, slots, P = _decode_setup(kv_lens, Hq, Hkv, seed=7, S=8)
    B = len(kv_lens)
    gd = Guard()
    Ka, Va, Kb, Vb = gd.fp8_cache(K8), gd.fp8_cache(V8), gd.fp8_cache(K8), gd.fp8_cache(V8)
    cos, sin = _rope()
    pt, mp = native.decode_partitions(max(kv_lens), B, Hkv, target_blocks=256)
    assert mp > 1
    w = (torch.randn(4096, Hq * D, device=DEV) / math.sqrt(Hq * D)).bfloat16()
    assert native.gemm_part_merge_ok(B, w, Hq, mp, torch.empty(1))
    ws_o = gd.alloc((B, Hq, mp, D), torch.float32, F32_SENT)
    ws_ml = gd.alloc((B, Hq, mp, 2), torch.float32, F32_SENT)
    ref_attn = gd.out((B, Hq * D))
    native.attn_decode_rope(P, pos, cos, sin, slots, Kb, Vb, bt, kvl, ref_attn, Hq, Hkv, D, pt, mp)
    ref = native.gemm_part(ref_attn, w).sum(0)
    attn = gd.out((B, Hq * D), fill=0.0)
    native.attn_decode_rope(P, pos, cos, sin, slots, Ka, Va, bt, kvl, attn, Hq, Hkv, D, pt, mp, ws_o=ws_o,
                            ws_ml=ws_ml, defer_merge=True)
    out = native.gemm_part_merge(attn, kvl, pt, mp, ws_o, ws_ml, Hq, w).sum(0)
    assert gd.intact()
    assert _same(Ka, Kb) and _same(Va, Vb)
    oracle = ref_attn.float() @ w.float().t()
    assert rel_err(ref, oracle) < 1e-4
    assert rel_err(out, oracle) < 2e-3, rel_err(out, oracle)


# ------------------------------------------------------------------------------------- 4. prefill attention
@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (8, 1), (4, 2), (2, 2)])
@pytest.mark.parametrize("q_lens,kv_lens", [([37], [37]), ([100, 64, 1], [100, 300, 129]), ([5, 70], [513, 70]),
                                            ([1], [1]), ([64, 65], [64, 200])])
def test_attn_prefill_fp8(native, q_lens, kv_lens, Hq, Hkv):
    """The fp8 paged causal prefill kernel (GB 4 / 2 / 1) vs the oracle: ragged tails, chunked prefill
    (q_len < kv_len), q_len = 1 rows (decoding rows of mixed steps)."""
    k16, v16, K8, V8, bt = _paged_fp8(kv_lens, Hkv, seed=21)
    gd = Guard()
    K8g, V8g = gd.fp8_cache(K8), gd.fp8_cache(V8)
    T = sum(q_lens)
    q = torch.randn(T, Hq * D, generator=torch.Generator().manual_seed(22)).bfloat16()
    cu = torch.tensor([0] + list(itertools.accumulate(q_lens)), dtype=torch.int32)
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    tiles = native.build_prefill_tiles(q_lens, Hq, Hkv).to(DEV)
    out = gd.out((T, Hq * D))
    native.attn_prefill(q.to(DEV), K8g, V8g, cu.to(DEV), kvl.to(DEV), tiles, out, Hq, Hkv, D, causal=True, paged=True,
                        block_tables=bt.to(DEV))
    assert gd.intact()
    assert _same(K8g, K8) and _same(V8g, V8)
    ref = _oracle(q, K8, V8, bt, kv_lens, cu, Hq)
    e = rel_err(out.cpu().reshape(T, Hq, D), ref)
    print("prefill fp8 rel_err %.3e" % e)
    assert e < 2e-2, e


def test_fp8_scale_checks(native):
    """Host-side checks on the scale tensors: shape, fp32, contiguous, same device."""
    k16, v16, K8, V8, bt = _paged_fp8([65], 1, seed=30)
    Kg, Vg = Fp8KV(K8.data.to(DEV), K8.scale.to(DEV)), Fp8KV(V8.data.to(DEV), V8.scale.to(DEV))
    q = torch.randn(1, 4 * D, device=DEV).bfloat16()
    out = torch.empty_like(q)
    kvl = torch.tensor([65], dtype=torch.int32, device=DEV)
    args = (bt.to(DEV), kvl, out, 4, 1, D, 4, 1)
    native.attn_decode(q, Kg, Vg, *args)
    bad = [Fp8KV(Kg.data, Kg.scale.double()), Fp8KV(Kg.data, Kg.scale[:, :, :32]),
           Fp8KV(Kg.data, Kg.scale.cpu()), Fp8KV(Kg.data, Kg.scale.transpose(0, 2).contiguous().transpose(0, 2))]
    for b in bad:
        with pytest.raises(ValueError):
            native.attn_decode(q, b, Vg, *args)
        with pytest.raises(ValueError):
            native.attn_decode(q, Kg, b, *args)
    with pytest.raises(ValueError):
        native.attn_decode(q, Kg, v16.to(DEV), *args)  # mixed formats


# ------------------------------------------------------------------------------------- 6. engine
def _engine(cfg, sd, device, graphs, mb=8):
    w = LlamaWeights.from_state_dict(cfg, sd, device)
    m = LlamaModel(cfg, w, device, max_positions=2048)
    return LLMEngine(m, num_blocks=64, max_batch=mb, max_prefill_tokens=300, max_model_len=2048, use_graphs=graphs,
                     kv_dtype="fp8")


@pytest.fixture(scope="module")
def tiny_llama():
    cfg = llama_tiny(vocab=1024, layers=2, hidden=512, heads=4, kv_heads=1, inter=512)
    return cfg, llama_state_dict(cfg, seed=3, std=0.05)


def _oracle_logits(cfg, sd, ids):
    """CPU oracle with the fp8 cache: logits [T, V] of every position of `ids` (one prefill)."""
    eng = _engine(cfg, sd, "cpu", graphs=False)
    n = len(ids)
    eng.bm.ensure(99, n + 1)
    tbl = eng.bm.table(99)
    slots = torch.tensor([tbl[q // 64] * 64 + q % 64 for q in range(n)], dtype=torch.int32)
    bt = torch.tensor([tbl + [0] * (eng.max_blocks - len(tbl))], dtype=torch.int32)
    meta = AttnMeta("prefill", torch.tensor([n], dtype=torch.int32), bt, cu_q=torch.tensor([0, n], dtype=torch.int32),
                    host_kv_lens=[n])
    inp = StepInput(torch.tensor(ids, dtype=torch.int32), torch.arange(n, dtype=torch.int32), slots, meta, None)
    return eng.model.forward(inp).float()


def _check_greedy(cfg, sd, prompts, outs, rel_tol=0.02):
    """The per-step top-1 margin rule of tests/test_e2e_gpu.py (teacher forced on the GPU's own tokens)."""
    exact = 0
    for pr, out in zip(prompts, outs):
        lg = _oracle_logits(cfg, sd, pr + out[:-1])
        for k, tok in enumerate(out):
            row = lg[len(pr) - 1 + k]
            top = float(row.max())
            gap = top - float(row[tok])
            spread = top - float(row.min())
            assert gap <= rel_tol * spread, (k, tok, int(row.argmax()), gap, spread)
            exact += int(gap == 0.0)
    return exact


def test_gpu_engine_fp8_cache_matches_cpu_greedy(native, tiny_llama):
    """GPU engine (graphs, async decode, mixed steps) with the fp8 cache vs the CPU engine with the fp8 cache."""
    cfg, sd = tiny_llama
    torch.manual_seed(0)
    prompts = [torch.randint(3, 1000, (n,)).tolist() for n in (5, 77, 130, 300, 513)]
    p = SamplingParams(max_new_tokens=6, do_sample=False, ignore_eos=True)
    eng = _engine(cfg, sd, "cuda", graphs=True)
    assert eng.stats["kv_dtype"] == "fp8" and isinstance(eng.model.kv_cache[0][0], Fp8KV)
    gpu = eng.generate(prompts, p)
    assert eng.bm.free_blocks() == 64 - 1  # every block back (block 0 is the scratch block)
    exact = _check_greedy(cfg, sd, prompts, gpu)
    assert exact >= 0.7 * sum(len(x) for x in gpu), exact


def test_graph_decode_equals_eager_fp8_cache(native, tiny_llama):
    cfg, sd = tiny_llama
    torch.manual_seed(1)
    prompts = [torch.randint(3, 1000, (n,)).tolist() for n in (9, 40, 200)]
    p = SamplingParams(max_new_tokens=10, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True)
    ea, eb = _engine(cfg, sd, "cuda", graphs=True), _engine(cfg, sd, "cuda", graphs=False)
    a = ea.generate(prompts, p, seeds=[1, 2, 3])
    b = eb.generate(prompts, p, seeds=[1, 2, 3])
    assert a == b
    assert ea.bm.free_blocks() == 63 and eb.bm.free_blocks() == 63


def test_batch1_mlp_engine_route_fp8_cache(native, tiny_llama):
    """One batch-1 run: the decode steps take the persistent mlp_engine launch, with the fp8 cache under it."""
    cfg, sd = tiny_llama
    torch.manual_seed(2)
    prompts = [torch.randint(3, 1000, (77,)).tolist()]
    eng = _engine(cfg, sd, "cuda", graphs=True)
    L0 = eng.model.w.layers[0]
    assert eng.model.be.mlp_engine_ok(1, L0["wgu"], L0["wdown"])
    out = eng.generate(prompts, SamplingParams(max_new_tokens=6, do_sample=False, ignore_eos=True))
    assert eng.stats.get("engine_faults", 0) == 0 and eng.bm.free_blocks() == 63
    _check_greedy(cfg, sd, prompts, out)
